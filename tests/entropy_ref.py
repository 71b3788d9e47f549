"""numpy statements of the entropy penalties of csrc/entropy.hip (functional.entropy_loss) for its
tests, and the inputs those tests share.  No torch.

Logits x [n, h, w, c] (NHWC here, as the kernel reads them).  Per pixel, d = x - max x, e = exp d,
Z = sum_k e in class order, p = e / Z, log p = d - log Z:

    H = -sum_k p_k log p_k        a term with p_k == 0 contributes 0 (torch's xlogy rule)
    h = min(H * (1 / ln c), 1)    S = sum_k p_k^2        b_j = -(1 / ln c) p_j (log p_j + H)
    entropy      phi = h                      dphi/dx_j = b_j
    robust       phi = (h^2 + 1e-8)^eta       dphi/dx_j = 2 eta h (h^2 + 1e-8)^(eta - 1) b_j
    max_squares  phi = -S / 2                 dphi/dx_j = -p_j (p_j - S)
    loss = sum_pixels phi / (n h w world), mean_entropy = sum_pixels h / (n h w world),
    dloss/dx = g dphi/dx / (n h w world); the gradient term of a class with p_j == 0 is 0.

``entropy(..., np.float64)`` is the yardstick (it equals torch fp64 autograd of
-(softmax * log_softmax).sum(1) / ln c and the two penalties of it: tests/test_entropy_cpu.py).
``entropy(..., np.float32)`` restates the kernel's own formulas: every product, sum and difference
rounded to fp32 on its own, sequential sums, fp32(1 / ln c), eta == 2 formed as a product; exp, log
and pow are correctly rounded there, so the file it records (tests/pinned/entropy_tol.json) is the
same on every machine.  (The kernel adds a row's even and odd classes on two lanes and joins them:
another summation order, which the tests' margin is there for.)"""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np

try:
    from tests.distill_ref import BF16_OUT, MARGIN, _soften, logits, to_bf16  # noqa: F401
except ImportError:  # run as a script: python tests/entropy_ref.py
    from distill_ref import BF16_OUT, MARGIN, _soften, logits, to_bf16  # noqa: F401

# (n, c, h, w)
SHAPES = [
    (2, 19, 8, 16),      # two full tiles, the c = 19 instantiation
    (1, 19, 13, 17),     # a tail tile, odd sizes
    (2, 7, 9, 40),       # runtime c, tiles crossing the image boundary
    (1, 2, 4, 4),        # the smallest c
    (1, 32, 4, 4),       # the largest c
    (1, 19, 1, 1),       # one pixel
    (1, 19, 64, 128),    # the real geometry
]
REAL = SHAPES[6]
PENALTIES = [("entropy", 2.0), ("robust", 2.0), ("max_squares", 2.0), ("robust", 0.5)]
# (shape, penalty, eta, dtype): every shape in both dtypes, the penalties taking turns; the real
# geometry under every penalty
CASES = [(s,) + PENALTIES[i % 4] + (d,) for i, s in enumerate(SHAPES) for d in ("f32", "bf16")]
CASES += [(REAL, "entropy", 2.0, "f32"), (REAL, "robust", 2.0, "bf16"), (REAL, "robust", 0.5, "f32")]
QUANTITIES = ("loss", "entropy", "grad", "map")
PINNED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pinned", "entropy_tol.json")


def key(shape, penalty, eta, dtype):
    n, c, h, w = shape
    return f"n{n}c{c}_{h}x{w}_{penalty}" + (f"_eta{eta:g}" if penalty == "robust" else "") + f"_{dtype}"


IDS = [key(*c) for c in CASES]


def _seq(t, dt):
    """Sum over the last axis in class order, every partial sum rounded to ``dt``."""
    acc = np.zeros(t.shape[:-1], dtype=dt)
    for k in range(t.shape[-1]):
        acc = (acc + t[..., k]).astype(dt)
    return acc


def entropy(x, penalty, eta=2.0, dt=np.float64, world=1, g=1.0):
    """(loss, mean_entropy, dloss/dx [n, h, w, c], h [n, h, w]) of NHWC logits ``x`` in ``dt``."""
    n, hh, ww, c = x.shape
    d, e, z, lz = _soften(x.astype(dt), 1.0, dt)
    inv = dt(1.0 / np.log(float(c)))
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        p = (e / z[..., None]).astype(dt)
        lp = (d - lz[..., None]).astype(dt)
        acc = _seq(np.where(p == 0, dt(0), (p * lp).astype(dt)).astype(dt), dt)
        sq = _seq((p * p).astype(dt), dt)
        ent = (-acc).astype(dt)
        hn = np.minimum((ent * inv).astype(dt), dt(1))
        if penalty == "max_squares":
            phi = (dt(-0.5) * sq).astype(dt)
            term = np.where(p == 0, dt(0), -(p * (p - sq[..., None]).astype(dt)).astype(dt)).astype(dt)
        else:
            base = np.where(p == 0, dt(0), -((p * (lp + ent[..., None]).astype(dt)).astype(dt) * inv).astype(dt)).astype(dt)
            if penalty == "entropy":
                phi, f = hn, np.ones_like(hn)
            elif penalty == "robust":
                u = ((hn * hn).astype(dt) + dt(1e-8)).astype(dt)
                if eta == 2.0:
                    phi, pw = (u * u).astype(dt), u
                else:  # correctly rounded: formed in fp64
                    phi = np.power(u.astype(np.float64), float(dt(eta))).astype(dt)
                    pw = np.power(u.astype(np.float64), float((dt(eta) - dt(1)).astype(dt))).astype(dt)
                f = (((dt(2) * dt(eta)).astype(dt) * hn).astype(dt) * pw).astype(dt)
            else:
                raise ValueError(penalty)
            term = (f[..., None] * base).astype(dt)
    coef = 1.0 / float(n * hh * ww * world)
    loss = dt(coef * float(np.add.accumulate(phi.reshape(-1), dtype=dt)[-1]))      # sequential
    ment = dt(coef * float(np.add.accumulate(hn.reshape(-1), dtype=dt)[-1]))
    grad = (dt(g * coef) * term).astype(dt)
    return loss, ment, grad, hn


# ------------------------------------------------------------------ special rows
def special_rows(c=19):
    """[1, 1, 4, c] fp32 (every value fits bf16): one logit at 200 above noise (entropy and gradient
    exactly 0 in fp32: the other exponentials underflow); a constant row (h = 1, gradient 0); a row
    with classes at -inf (finite loss, gradient 0 there); two equal maxima."""
    x = to_bf16(logits((1, 1, 4, c), 7, "f32"))
    x[0, 0, 0, 3] = 200.0
    x[0, 0, 1, :] = 1.5
    x[0, 0, 2, [1, 4, c - 1]] = -np.inf
    x[0, 0, 3, [2, 9 % c]] = 6.0
    x[0, 0, 3] = np.minimum(x[0, 0, 3], 6.0)
    return x


# ------------------------------------------------------------------ shared cases
def seed_of(k):
    return 2000 + sorted(IDS).index(k)


@functools.lru_cache(maxsize=None)
def case(shape, penalty, eta, dtype):
    """Computed once per case and left unchanged: the input (an fp32 array holding values of its
    dtype), the fp64 yardstick and the fp32 restatement."""
    n, c, h, w = shape
    x = logits((n, h, w, c), seed_of(key(shape, penalty, eta, dtype)), dtype)
    l64, e64, g64, m64 = entropy(x, penalty, eta)
    l32, e32, g32, m32 = entropy(x, penalty, eta, np.float32)
    return SimpleNamespace(x=x, loss64=float(l64), ent64=float(e64), grad64=g64, map64=m64,
                           loss32=l32, ent32=e32, grad32=g32, map32=m32)


def _ulp(v):
    return float(np.spacing(np.float32(abs(v))))


def tolerance(c):
    """{"loss", "entropy", "grad", "map"} before the margin: max(error of the fp32 restatement against
    fp64, one fp32 ulp of the reference value); the gradient's and the map's in absolute terms at
    their largest element."""
    gmax, mmax = float(np.abs(c.grad64).max()), float(np.abs(c.map64).max())
    return {"loss": max(abs(float(c.loss32) - c.loss64), _ulp(c.loss64)),
            "entropy": max(abs(float(c.ent32) - c.ent64), _ulp(c.ent64)),
            "grad": max(float(np.abs(c.grad32.astype(np.float64) - c.grad64).max()), _ulp(gmax)),
            "map": max(float(np.abs(c.map32.astype(np.float64) - c.map64).max()), _ulp(mmax))}


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
