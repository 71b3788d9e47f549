"""AdvEnt's discriminator input (include/rtsds_hip.h: rtsds_upselfinfo_fwd / _bwd, functional.upsample_self_information)
stated as formulas in the vocabulary of tests/route_compare.py: ``reference(case, inputs, dtype)`` returns the outputs
``y`` and ``dx`` as route_compare.Out.  float64 is the statement; the float32 evaluation follows the kernel's formulas
and serves the tolerance alone.

Per output pixel of the resized head, z = the bilinear resize (align_corners=False, tests/resize_route_ref.py):

    d_k = z_k - max z      e_k = exp d_k      S = sum_k e_k      p_k = e_k / S      L_k = log S - d_k  (= -ln p_k)
    I_k = p_k L_k / ln c                       0 where e_k == 0 (a class at -inf)
    a_k = (L_k - 1) / ln c  (= dI_k / dp_k)    u_k = dy_k a_k     dz_j = p_j (u_j - sum_k p_k u_k)
    dx  = adjoint of the resize, of dz

which is ADVENT's prob_2_entropy, -p log2(p + 1e-30) / log2(c), without the epsilon (tests/test_selfinfo_cpu.py
compares the two).  A bf16 case takes z = bf16(resize in the kernel's fp32 operations) as certain -- the header defines z
as "rounded to the activation dtype exactly as rtsds_bilinear_fwd stores it", the rule of resize_route_ref._probs -- and
is float64 from there on; nothing else is rounded on the way (dz stays fp32 until the adjoint has summed it), so no
element is excluded: there is no mask, no argmax and no doubtful intermediate rounding.

Tolerances (route_compare.tolerance): m * max(E32, 2^-23 M), m = max(8, ceil(log2(N) / 2)); y is elementwise over a sum
of c exponentials (M = max |I|, N = c); dx is a sum (M = adjoint(|p| (|u| + sum |p u|)), N = adjoint terms * (c + 1)),
as the softmax sibling's ``usb``; 2^-8 |ref| per element on top for a bf16 output.  Recorded once on the CPU by
record() into tests/pinned/selfinfo_tol.json (python -m tests.selfinfo_ref)."""
import functools
import json
import math
import os

import numpy as np
import torch

from .bn_bits_cases import BF16, F32, pattern
from .resize_bits_cases import _scale
from .resize_route_ref import _adj_terms, adjoint, adjoint_less, resize, resize_fp32
from .route_compare import Out, bf16r, host, tolerance

TOL_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pinned", "selfinfo_tol.json")

# (n, c, hi, wi) -> (ho, wo), what it covers, and the backward planner's branch: the tile is the widest of 64, 32, ..
# input columns whose LDS fits (upsm_tiling), then narrowed to the widest width that saves a pass of the 256-pixel
# per-pixel loop where that pays (upsi_trim); tw = the width taken, cap = its largest segment in output columns
GEOS = [
    ((2, 19, 16, 32), (128, 256)),   # x8, the compile-time 19 classes; tw = 64 fits, one tile of 32 columns, cap 256: one pass
    ((1, 19, 13, 17), (97, 129)),    # odd sizes, a non-integer factor
    ((1, 19, 9, 17), (64, 128)),     # DeepLab's 65 x 129 -> 512 x 1024 ratio in small
    ((2, 7, 9, 40), (64, 96)),       # runtime class count
    ((1, 19, 8, 40), (24, 300)),     # two forward column tiles, the last ragged (44 pixels); backward trimmed 64 -> 33 (cap 300 -> 253)
    ((1, 2, 4, 4), (8, 8)),          # the smallest class count
    ((1, 32, 4, 4), (8, 8)),         # the largest
    ((1, 19, 8, 8), (8, 8)),         # identity
    ((1, 19, 2, 4200), (4, 256)),    # staged rows over the LDS budget: the unstaged forward; 66 backward tiles (tw = 64, cap 8)
    ((1, 19, 3, 70), (6, 140)),      # two backward tiles of tw = 64, the second ragged (6 columns)
    # the planner's narrower tiles by LDS: 32 classes and a steeper and steeper width factor, so that the fp32 segment
    # of a tile of 2 tw columns no longer fits the LDS cap and the one of tw columns does (cap 197 .. 242: one pass)
    ((1, 32, 2, 64), (4, 384)),      # x6: tw = 32
    ((1, 32, 2, 32), (4, 384)),      # x12: tw = 16
    ((1, 32, 2, 16), (4, 384)),      # x24: tw = 8
    ((1, 32, 2, 8), (4, 384)),       # x48: tw = 4
    ((1, 32, 2, 4), (4, 384)),       # x96: tw = 2
    ((1, 32, 2, 2), (4, 384)),       # x192: tw = 1, cap 290: two passes, and no width left to trim to
    # the benchmark's branch in small (64 x 128 -> 512 x 1024 takes the same widths): x8 at the compile-time 19 classes,
    # tw = 64 does not fit (55 KB), tw = 32 does with cap 268, trimmed to 30 (cap 252, one pass): tiles of 30, 30, 4
    ((1, 19, 2, 64), (4, 512)),
    # a trim from three passes to two with the runtime class count: tw = 64 fits with cap 518, trimmed to 62 (cap 508)
    ((1, 7, 2, 128), (4, 1024)),
    # two passes that no narrower tile improves: x150, tw = 2 (cap 377), and tw = 1 would be one pass per column
    ((1, 19, 2, 4), (4, 600)),
]
# the geometry no tile of which fits: one input column spreading over all 400 output columns at 32 classes
UNSUPPORTED_BWD = ((1, 32, 2, 1), (4, 400))
IDENTITY = GEOS[7]
# the pitches the Python layer uses (y_ld = 32, dy dense), and on three geometries a dense y with a pitched dy
PITCHED = (GEOS[1], GEOS[3], GEOS[6], GEOS[9])


def _case(geo, dt, yld=32, dyld=None):
    (n, c, hi, wi), (ho, wo) = geo
    return dict(n=n, c=c, hi=hi, wi=wi, ho=ho, wo=wo, dt=dt, yld=yld, dyld=dyld or c)


CASES = [_case(g, dt) for g in GEOS for dt in (F32, BF16)]
CASES += [_case(g, dt, yld=g[0][1], dyld=min(32, g[0][1] + 5) if g[0][1] < 32 else 37) for g in PITCHED for dt in (F32, BF16)]


def case_id(k):
    return (f"n{k['n']}c{k['c']}_{k['hi']}x{k['wi']}_to_{k['ho']}x{k['wo']}_yld{k['yld']}_dyld{k['dyld']}_"
            + ("bf16" if k["dt"] == BF16 else "f32"))


IDS = [case_id(k) for k in CASES]
assert len(set(IDS)) == len(IDS)


def host_inputs(k):
    """The head x [n][hi][wi][c] in [-8, 8) and the upstream gradient dy [n][ho][wo][dyld] in [-2, 2), fp32 arrays from
    the flat element index (a bf16 case rounds them on the way)."""
    return dict(x=pattern(k["n"] * k["hi"] * k["wi"] * k["c"], 1), dy=pattern(k["n"] * k["ho"] * k["wo"] * k["dyld"], 4) / 4)


def _seq_sum(t):
    """Sum over the last axis in class order (float32: every partial sum rounded, as the kernel adds)."""
    acc = torch.zeros(t.shape[:-1], dtype=t.dtype)
    for j in range(t.shape[-1]):
        acc = acc + t[..., j]
    return acc


def logits(k, x, dtype):
    """z [n][ho][wo][c] of the head x [n][hi][wi][c] (values of the case's dtype, held in ``dtype``)."""
    return bf16r(resize_fp32(x, k)).to(dtype) if k["dt"] == BF16 else resize(x, k, dtype)


def terms(z, c, dtype):
    """(p, L, 1 / ln c, e) of logits z in ``dtype``; float32 takes the kernel's route: p = e * (1 / S), fp32(1 / ln c)."""
    d = z - z.max(-1, keepdim=True).values
    e = torch.exp(d)
    S = _seq_sum(e)[..., None]
    p = e * (1 / S) if dtype == torch.float32 else e / S
    inv = torch.tensor(1.0 / math.log(c), dtype=dtype)
    return p, torch.log(S) - d, inv, e


def self_information(z, c, dtype, drop=None):
    """I of logits z.  drop: that class left out of the sum S (a wrong kernel, for Out.dropped)."""
    if drop is not None:
        d = z - z.max(-1, keepdim=True).values
        e = torch.exp(d)
        S = (_seq_sum(e) - e[..., drop])[..., None]
        p, L, inv = e / S, torch.log(S) - d, torch.tensor(1.0 / math.log(c), dtype=dtype)
    else:
        p, L, inv, e = terms(z, c, dtype)
    return torch.where(e == 0, torch.zeros_like(p), p * L * inv)


def logit_gradient(z, dy, c, dtype, wrong=None):
    """(dz, M) of logits z and the upstream gradient dy; M = |p| (|u| + sum |p u|).  wrong: a mistaken kernel, for
    the tests that the comparison rejects it -- "no_minus_one": a_k = L_k / ln c; "short_dot": class 0 left out of
    sum_k p_k u_k."""
    p, L, inv, e = terms(z, c, dtype)
    a = torch.where(e == 0, torch.zeros_like(p), ((L if wrong == "no_minus_one" else L - 1)) * inv)
    u = dy * a
    pu = p * u
    dot = _seq_sum(pu[..., 1:] if wrong == "short_dot" else pu)[..., None]
    return p * (u - dot), p.abs() * (u.abs() + _seq_sum(pu.abs())[..., None])


def reference(k, h, dtype=torch.float64, tols=None, wrong=None):
    """{"y", "dx"} of one case.  y is stated whole, [n][ho][wo][y_ld]: its columns c.. hold exact zeros."""
    n, hi, wi, c, ho, wo, dt = k["n"], k["hi"], k["wi"], k["c"], k["ho"], k["wo"], k["dt"]
    x = host(h["x"], dt, dtype).view(n, hi, wi, c)
    dy = host(h["dy"], dt, dtype).view(n, ho, wo, k["dyld"])[..., :c]
    z = logits(k, x, dtype)
    y, yl = torch.zeros((n, ho, wo, k["yld"]), dtype=dtype), torch.zeros((n, ho, wo, k["yld"]), dtype=dtype)
    y[..., :c], yl[..., :c] = self_information(z, c, dtype), self_information(z, c, dtype, drop=0)
    fixed = torch.zeros(y.shape, dtype=torch.bool)
    fixed[..., c:] = True
    dz, M = logit_gradient(z, dy, c, dtype, wrong)
    return dict(y=Out(y, None, c, bf16=dt == BF16, fixed=fixed, dropped=yl),
                dx=Out(adjoint(dz, k, dtype), adjoint(M, k, dtype), _adj_terms(k) * (c + 1), bf16=dt == BF16,
                       dropped=adjoint_less(dz, k, dtype)))


@functools.lru_cache(maxsize=None)
def case(i):
    """(host inputs, float64 reference) of CASES[i], computed once and left unchanged."""
    h = host_inputs(CASES[i])
    return h, reference(CASES[i], h)


def special_rows(c=19):
    """Four rows of logits [4][c] (fp32 values that fit bf16): one logit at 200 above noise (I = 0 everywhere: p is 1
    there and underflows to 0 elsewhere); a constant row (p = 1 / c, I = 1 / c); classes at -inf (I = 0 there, finite
    elsewhere); two equal maxima."""
    x = torch.from_numpy(pattern(4 * c, 3).reshape(4, c) / 4).to(torch.bfloat16).float().numpy()
    x[0, 3] = 200.0
    x[1, :] = 1.5
    x[2, [1, 4, c - 1]] = -np.inf
    x[3, [2, 9 % c]] = 6.0
    x[3] = np.minimum(x[3], 6.0)
    return x


# The special rows reach the kernel through a resize in which no tap has weight zero (0 * -inf is NaN in any bilinear
# resize, torch's included: a class at -inf survives only where every tap that is read has a weight): 2 x 8 -> 1 x 4,
# every output pixel the mean of a 2 x 2 block, the four pixels of block j all holding row j.  So z is the rows
# themselves, exactly (fmaf(0.5, v, 0.5 v) = v), and each input pixel receives a quarter of its block's dz.
def special_case(c, dt):
    return dict(n=1, c=c, hi=2, wi=8, ho=1, wo=4, dt=dt, yld=32, dyld=c)


def special_head(c=19):
    """The head [1][2][8][c] of special_case."""
    return np.ascontiguousarray(np.repeat(np.repeat(special_rows(c)[None, None], 2, axis=2), 2, axis=1))


def special_reference(c, dy, dtype=torch.float64):
    """(I [4][c], dx [1][2][8][c]) of special_head under the upstream gradient dy [4][c]."""
    z, dy = torch.from_numpy(special_rows(c)).to(dtype), torch.as_tensor(dy).to(dtype)
    dz, _ = logit_gradient(z, dy, c, dtype)
    return self_information(z, c, dtype), (dz / 4).repeat_interleave(2, 0)[None, None].expand(1, 2, 8, c).contiguous()


def record():
    """The pinned file's content: per case and output, the tolerance at 4 significant digits."""
    out = {}
    for i, k in enumerate(CASES):
        h, r64 = case(i)
        r32 = reference(k, h, torch.float32)
        out[IDS[i]] = {name: float(f"{tolerance(r64[name], r32[name]):.4g}") for name in ("y", "dx")}
    return out


def pinned():
    with open(TOL_PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(TOL_PATH, "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
