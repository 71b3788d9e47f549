"""numpy statements of the distillation loss of csrc/distill.hip (functional.distill_kl) for its
tests, and the inputs those tests share.  No torch.

Student s [n, hs, ws, c] and teacher t [n, ht, wt, c] (NHWC here, as the kernel reads them).  The
teacher is resampled onto the student's grid (bilinear, align_corners=False, not antialiased, any
ratio), then per student pixel, with a = s/T, b = u/T, q = softmax(a), p = softmax(b):

    KL   = sum_k p_k (log p_k - log q_k)        a term with p_k == 0 contributes 0 (torch's xlogy rule)
    loss = T^2 * sum_pixels KL / (n hs ws world)
    dloss/ds_k = g * T * (q_k - p_k) / (n hs ws world)

``distill(..., np.float64)`` is the yardstick (it equals F.interpolate -> F.kl_div(log_softmax(s/T),
softmax(u/T), 'sum') * T^2 / N in torch fp64 with autograd: tests/test_distill_cpu.py).
``distill(..., np.float32)`` restates the kernel's own formulas: the source scale and bil_src's taps
in fp32, bil_mix's fma order, sequential fp32 sums, fp32(1/T); exp and log are correctly rounded
there, so the file it records (tests/pinned/distill_tol.json) is the same on every machine."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np

# (n, c, hs, ws, ht, wt): the student's grid <- the teacher's
SHAPES = [
    (2, 19, 8, 16, 9, 17),       # DeepLab -> BiSeNet at a 64x128 input: c = 19 instantiation, slight downsample, image stride
    (1, 19, 13, 17, 13, 17),     # identity taps, odd sizes
    (2, 7, 9, 40, 5, 21),        # runtime c, a non-integer upsample
    (1, 32, 4, 4, 7, 3),         # the largest c, down in H and up in W
    (1, 2, 4, 4, 2, 2),          # the smallest c
    (1, 19, 3, 300, 5, 77),      # a row wider than one tile, with a tail
    (1, 19, 2, 260, 2, 4200),    # a source span too wide to stage
    (1, 19, 64, 128, 65, 129),   # the real geometry
    (1, 5, 2, 3, 3, 2000),       # runtime c with a span too wide to stage (the two planning branches, crossed)
]
REAL = SHAPES[7]
TEMPS = [1.0, 0.5, 4.0]
# (shape, T, student dtype, teacher dtype): every shape in both dtypes, T taking turns; the real
# geometry at every T; one fp32-student / bf16-teacher pair
CASES = [(s, TEMPS[i % 3], d, d) for i, s in enumerate(SHAPES) for d in ("f32", "bf16")]
CASES += [(REAL, 1.0, "f32", "f32"), (REAL, 4.0, "bf16", "bf16"), (SHAPES[0], 4.0, "f32", "bf16")]
MARGIN = 8.0
BF16_OUT = 2.0 ** -8   # per element of a bf16 output: one bf16 rounding plus one boundary flip
PINNED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pinned", "distill_tol.json")


def key(shape, temp, sd, td):
    n, c, hs, ws, ht, wt = shape
    return f"n{n}c{c}_{hs}x{ws}_from_{ht}x{wt}_T{temp:g}_{sd}_{td}"


IDS = [key(*c) for c in CASES]


def to_bf16(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def logits(shape, seed, dtype):
    """Seeded logits of standard deviation 4, exactly representable in ``dtype``; fp32 array."""
    x = (4.0 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)
    return to_bf16(x) if dtype == "bf16" else x


# ------------------------------------------------------------------ the resample
def taps(out, inn, dt):
    """ATen's align_corners=False taps (common.h bil_src) of every output index, formed in ``dt``:
    (i0, i1, l0, l1).  The source scale is in / out in ``dt`` (functional._src_scale in fp32)."""
    scale = dt(inn) / dt(out)
    src = scale * (np.arange(out).astype(dt) + dt(0.5)) - dt(0.5)
    src = np.maximum(src, dt(0))
    i0 = np.minimum(src.astype(np.int64), inn - 1)
    i1 = i0 + (i0 < inn - 1)
    l1 = (src - i0.astype(dt)).astype(dt)
    return i0, i1, (dt(1) - l1).astype(dt), l1


def _fma(a, b, c, dt):
    """a * b + c rounded once to ``dt`` (fp32: formed in fp64, where the product is exact)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(dt)


def resample(t, hs, ws, dt):
    """u [n, hs, ws, c] in ``dt``: common.h bil_mix -- width inner, height outer, fma order -- with a
    tap of weight zero left out (distill.hip kd_mix; the same values for finite taps)."""
    n, ht, wt, c = t.shape
    t = t.astype(dt)
    h0, h1, lh0, lh1 = taps(hs, ht, dt)
    w0, w1, lw0, lw1 = taps(ws, wt, dt)
    lw0, lw1 = lw0[None, None, :, None], lw1[None, None, :, None]
    lh0, lh1 = lh0[None, :, None, None], lh1[None, :, None, None]
    top, bot = t[:, h0], t[:, h1]
    with np.errstate(invalid="ignore"):  # a tap of weight zero is left out (an infinity under it would give NaN)
        t0 = np.where(lw1 == 0, top[:, :, w0], _fma(lw1, top[:, :, w1], (lw0 * top[:, :, w0]).astype(dt), dt))
        t1 = np.where(lw1 == 0, bot[:, :, w0], _fma(lw1, bot[:, :, w1], (lw0 * bot[:, :, w0]).astype(dt), dt))
        return np.where(lh1 == 0, t0, _fma(lh1, t1, (lh0 * t0).astype(dt), dt))


# ------------------------------------------------------------------ the loss
def _soften(x, inv_temp, dt):
    """(d, e, z, lz): d = x * inv_temp - max, e = exp(d), z = sum_k e in class order, lz = log z."""
    v = (x * dt(inv_temp)).astype(dt)
    d = (v - v.max(-1, keepdims=True)).astype(dt)
    with np.errstate(under="ignore"):
        e = np.exp(d.astype(np.float64)).astype(dt)
    z = np.zeros(d.shape[:-1], dtype=dt)
    for k in range(d.shape[-1]):
        z = (z + e[..., k]).astype(dt)
    return d, e, z, np.log(z.astype(np.float64)).astype(dt)


def distill(s, t, temp, dt=np.float64, world=1, g=1.0):
    """(loss, dloss/ds [n, hs, ws, c], agree, u) of NHWC student ``s`` and teacher ``t`` in ``dt``."""
    n, hs, ws, c = s.shape
    assert t.shape[0] == n and t.shape[3] == c
    u = resample(t, hs, ws, dt)
    inv_temp = np.float32(1.0 / temp) if dt == np.float32 else 1.0 / temp
    da, ea, za, lza = _soften(s.astype(dt), inv_temp, dt)
    db, eb, zb, lzb = _soften(u, inv_temp, dt)
    q, p = (ea / za[..., None]).astype(dt), (eb / zb[..., None]).astype(dt)
    with np.errstate(invalid="ignore"):
        diff = ((db - lzb[..., None]).astype(dt) - (da - lza[..., None]).astype(dt)).astype(dt)
        term = np.where(p == 0, dt(0), (p * diff).astype(dt)).astype(dt)
    kl = np.zeros(term.shape[:-1], dtype=dt)
    for k in range(c):
        kl = (kl + term[..., k]).astype(dt)
    total = np.add.accumulate(kl.reshape(-1), dtype=dt)[-1]            # sequential
    pixels = float(n * hs * ws * world)
    loss = dt(temp * temp / pixels * float(total))
    scale = dt(g * temp / pixels)
    grad = (scale * (q - p).astype(dt)).astype(dt)
    agree = int((np.argmax(s, -1) == np.argmax(u, -1)).sum())
    return loss, grad, agree, u


def top_gap(x):
    """Per row, the distance between the two largest values."""
    srt = np.sort(x, -1)
    return srt[..., -1] - srt[..., -2]


# ------------------------------------------------------------------ shared cases
# Seeds for which no resampled teacher row has its two largest values closer than 1e-4 or than four
# times the resample's own fp32 error (so `agree` is exact; premise checked in test_distill_cpu.py)
SEEDS = {"n1c19_2x260_from_2x4200_T1_f32_f32": 193, "n1c19_2x260_from_2x4200_T1_bf16_bf16": 206,
         "n1c19_64x128_from_65x129_T0.5_f32_f32": 1}


def seed_of(k):
    return SEEDS.get(k, 0) + 1000 * (1 + sorted(IDS).index(k))


def tie_margin(c):
    """(smallest top gap of u, max |u32 - u64|) of a case; identity taps are exact, their ties too."""
    return float(top_gap(c.u64).min()), float(np.abs(c.u32.astype(np.float64) - c.u64).max())


@functools.lru_cache(maxsize=None)
def case(shape, temp, sd, td):
    """Computed once per case and left unchanged: inputs (fp32 arrays holding values of their
    dtype), the fp64 yardstick and the fp32 restatement."""
    n, c, hs, ws, ht, wt = shape
    seed = seed_of(key(shape, temp, sd, td))
    s = logits((n, hs, ws, c), seed, sd)
    t = logits((n, ht, wt, c), seed + 1, td)
    l64, g64, a64, u64 = distill(s, t, temp)
    l32, g32, a32, u32 = distill(s, t, temp, np.float32)
    return SimpleNamespace(s=s, t=t, loss64=float(l64), grad64=g64, agree=a64, u64=u64, loss32=l32, grad32=g32, agree32=a32, u32=u32)


def tolerance(c):
    """{"loss", "grad"} before the margin: max(error of the fp32 restatement against fp64, one fp32
    ulp of the reference value); the gradient's in absolute terms at its largest element."""
    gmax = float(np.abs(c.grad64).max())
    return {"loss": max(abs(float(c.loss32) - c.loss64), float(np.spacing(np.float32(c.loss64)))),
            "grad": max(float(np.abs(c.grad32.astype(np.float64) - c.grad64).max()), float(np.spacing(np.float32(gmax))))}


def record():
    """The pinned file's content: 4 significant digits per figure."""
    return {k: {q: float(f"{v:.4g}") for q, v in tolerance(case(*c)).items()} for k, c in zip(IDS, CASES)}


def pinned():
    with open(PINNED_PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(PINNED_PATH, "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
