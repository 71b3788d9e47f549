"""The resize routes of tests/resize_bits_cases.py stated as formulas (include/rtsds_hip.h: bilinear resize,
discriminator input, multi-scale / flip evaluation): ``reference(case, inputs, dtype)`` returns every output
the driver pins, by the same names, as tests/route_compare.Out.  float64 is the reference; float32 serves
the tolerance alone.  Source index and weights follow ATen's align_corners=False rule from the fp32 scales
the driver passes: src = max(scale * (o + 0.5) - 0.5, 0), i0 = min(floor(src), in - 1), i1 = min(i0 + 1,
in - 1), l1 = src - i0, l0 = 1 - l1 (rtsds_amd/csrc/common.h bil_src); the backward is the exact adjoint.
A pitched output is stated whole: the columns outside the channel slice hold UNWRITTEN exactly.

Intermediate roundings (bf16 cases).  The header defines the fused kernels as bit-identical to unfused
chains, so what a chain stores between its kernels is part of the operation:
  rtsds_bilinear_fwd_scaled: "each product rounded to [the activation dtype] as rtsds_chscale_fwd mode 0
    stores it" (include/rtsds_hip.h) -- one fp32 multiply each, so the stored value is known to the bit.
  rtsds_upsoftmax_fwd / rtsds_upsoftmax_acc: "the logits are the bilinear_fwd values rounded to T"
    (rtsds_amd/csrc/resize.hip, the comment under "fused resize + softmax"; upsm_probs).
  rtsds_upsoftmax_bwd: "the softmax backward T(p_k (dp_k - sum_j p_j dp_j))" (same comment) is stored as T
    before the resize adjoint reads it.
A tolerance cannot decide the rounding of those two: a row of 19 logits within an fp32 error of a bf16
boundary is a few per cent of all rows, far over the exclusion cap.  The unit documents their fp32
expressions for exactly this purpose -- bil_src and bil_mix ("explicit fma order ... the same logits bit for
bit", common.h) and the chain's softmax backward (dot = fmaf(dy_k, y_k, dot) in class order, then
y_k * (dy_k - dot); rtsds_amd/csrc/chan.hip px_softmax_bwd, resize.hip upsoftmax_bwd_w_kernel) -- so a bf16
case states these two intermediates by those expressions with each fp32 operation's rounding, takes their
bf16 rounding as certain, and is float64 from there on.  The fp32 cases round nothing.
"""
import math

import torch

from .bn_bits_cases import BF16, UNWRITTEN
from .resize_bits_cases import _scale
from .route_compare import Out, bf16r, host, round_op


def f32(t):
    """t rounded to fp32, in float64."""
    return t.float().double()


def fma32(a, b, c):
    """fp32 fmaf(a, b, c) of fp32 values held in float64 (the product of two fp32 numbers is exact there)."""
    return f32(a * b + c)


def taps(out, inn, scale, dtype):
    """(i0, i1, l0, l1) of every output index, computed in ``dtype`` from the fp32 scale."""
    o = torch.arange(out, dtype=dtype)
    src = (torch.tensor(scale, dtype=dtype) * (o + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().clamp_max(inn - 1)
    l1 = src - i0
    i0 = i0.long()
    return i0, (i0 + 1).clamp_max(inn - 1), 1 - l1, l1


def taps_fp32(out, inn, scale):
    """The same exactly as the kernels form them (common.h bil_src: src = fmaf(o + 0.5, scale, -0.5) after
    the compiler's contraction, every other operation a single fp32 one), in float64."""
    o = torch.arange(out, dtype=torch.float64)
    src = f32(scale * (o + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().clamp_max(inn - 1)
    l1 = f32(src - i0)
    i0 = i0.long()
    return i0, (i0 + 1).clamp_max(inn - 1), f32(1 - l1), l1


def matrix(out, inn, scale, dtype):
    """The [out][in] interpolation matrix of one axis."""
    i0, i1, l0, l1 = taps(out, inn, scale, dtype)
    W = torch.zeros((out, inn), dtype=dtype)
    r = torch.arange(out)
    W.index_put_((r, i0), l0, accumulate=True)
    W.index_put_((r, i1), l1, accumulate=True)
    return W


def _mats(k, dtype):
    return (matrix(k["ho"], k["hi"], _scale(k["hi"], k["ho"]), dtype), matrix(k["wo"], k["wi"], _scale(k["wi"], k["wo"]), dtype))


def resize(x, k, dtype):
    """x [n][hi][wi][c] -> [n][ho][wo][c]."""
    Wh, Ww = _mats(k, dtype)
    return torch.einsum("ph,nhwc,qw->npqc", Wh, x, Ww)


def adjoint(dy, k, dtype):
    """dy [n][ho][wo][c] -> [n][hi][wi][c]: the transpose of resize."""
    Wh, Ww = _mats(k, dtype)
    return torch.einsum("ph,npqc,qw->nhwc", Wh, dy, Ww)


def adjoint_less(dy, k, dtype):
    """adjoint(dy) with, per input pixel, the term of its heaviest output pixel left out."""
    Wh, Ww = _mats(k, dtype)
    ph, qw = Wh.argmax(0), Ww.argmax(0)
    term = Wh[ph, torch.arange(k["hi"])][None, :, None, None] * Ww[qw, torch.arange(k["wi"])][None, None, :, None] * dy[:, ph][:, :, qw]
    return adjoint(dy, k, dtype) - term


def _adj_terms(k):
    return math.ceil(2 * k["ho"] / k["hi"] + 2) * math.ceil(2 * k["wo"] / k["wi"] + 2)


def resize_fp32(x, k):
    """The resized values exactly as rtsds_bilinear_fwd forms them in fp32 (bil_src, bil_mix), in float64."""
    h0, h1, lh0, lh1 = taps_fp32(k["ho"], k["hi"], _scale(k["hi"], k["ho"]))
    w0, w1, lw0, lw1 = taps_fp32(k["wo"], k["wi"], _scale(k["wi"], k["wo"]))
    x = x.double()
    lh0, lh1 = lh0[None, :, None, None], lh1[None, :, None, None]
    lw0, lw1 = lw0[None, None, :, None], lw1[None, None, :, None]
    r0, r1 = x[:, h0], x[:, h1]
    t0 = fma32(lw1, r0[:, :, w1], f32(lw0 * r0[:, :, w0]))
    t1 = fma32(lw1, r1[:, :, w1], f32(lw0 * r1[:, :, w0]))
    return fma32(lh1, t1, f32(lh0 * t0))


def _pitched(v, k, ld, off, dtype):
    n, ho, wo, c = v.shape
    if ld == c:
        return v.contiguous(), None
    full = torch.full((n, ho, wo, ld), UNWRITTEN, dtype=dtype)
    fixed = torch.ones((n, ho, wo, ld), dtype=torch.bool)
    full[..., off:off + c] = v
    fixed[..., off:off + c] = False
    return full, fixed


def supported(k):
    """False for the case whose entry point returns RTSDS_ERR_UNSUPPORTED: the scaled downsample."""
    return not (k["kind"] == "fwd" and k["s"] and k["ho"] < k["hi"])


def fwd(k, h, dtype, tols=None):
    n, hi, wi, c, dt = k["n"], k["hi"], k["wi"], k["c"], k["dt"]
    x = host(h["x"], dt, dtype).view(n, hi, wi, c)
    for s in ("s1", "s2"):
        if h[s] is not None:
            x = round_op(x * host(h[s], dt, dtype).view(n, 1, 1, c), dt)
    v, fixed = _pitched(resize(x, k, dtype), k, k["ld"] or c, k["off"], dtype)
    return dict(y=Out(v, None, 4, bf16=dt == BF16, fixed=fixed))


def bwd(k, h, dtype, tols=None):
    n, ho, wo, c, dt = k["n"], k["ho"], k["wo"], k["c"], k["dt"]
    ld = k["ld"] or c
    dy = host(h["dy"], dt, dtype).view(n, ho, wo, ld)[..., k["off"]:k["off"] + c]
    return dict(dx=Out(adjoint(dy, k, dtype), adjoint(dy.abs(), k, dtype), _adj_terms(k), bf16=dt == BF16,
                       dropped=adjoint_less(dy, k, dtype)))


def _probs(k, h, dtype):
    n, hi, wi, c, dt = k["n"], k["hi"], k["wi"], k["c"], k["dt"]
    x = host(h["x"], dt, dtype).view(n, hi, wi, c)
    z = bf16r(resize_fp32(x, k)).to(dtype) if dt == BF16 else resize(x, k, dtype)
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    less = e / (e.sum(-1, keepdim=True) - e[..., :1])   # class 0 left out of the sum
    less[..., 0] = (e / e.sum(-1, keepdim=True))[..., 0]
    return e / e.sum(-1, keepdim=True), less, z


def usf(k, h, dtype, tols=None):
    p, less, _ = _probs(k, h, dtype)
    n, ho, wo, c = p.shape
    y, yl = torch.zeros((n, ho, wo, k["yld"]), dtype=dtype), torch.zeros((n, ho, wo, k["yld"]), dtype=dtype)
    y[..., :c], yl[..., :c] = p, less
    fixed = torch.zeros(y.shape, dtype=torch.bool)
    fixed[..., c:] = True
    return dict(y=Out(y, None, c, bf16=k["dt"] == BF16, fixed=fixed, dropped=yl))


def usa(k, h, dtype, tols=None):
    p, less, z = _probs(k, h, dtype)
    n, ho, wo, c = p.shape
    if k["flip"]:
        p, less, z = p.flip(2), less.flip(2), z.flip(2)
    M, a0 = p.abs(), torch.zeros_like(p)
    if k["acc"]:
        a0 = host(h["acc0"], 0, dtype).view(n, ho, wo, c)
        p, less, M = a0 + p, a0 + less, a0.abs() + M
    outs = dict(acc=Out(p, M, c, dropped=less))
    if k["pred"]:
        win = p.argmax(-1, keepdim=True)                               # torch.argmax: the first of equal values
        accept = None
        if tols is not None:
            # a class within twice the tolerance of the maximum may win -- but not one whose operands (resized
            # logit, old sum) are the winner's own: the kernel's values are then equal too and the first wins
            twin = (z == z.gather(-1, win)) & (a0 == a0.gather(-1, win))
            near = (p >= p.gather(-1, win) - 2 * tols["acc"]) & ~twin
            accept = near.scatter(-1, win, True).reshape(-1, c)
        outs["pred"] = Out(win[..., 0], exact=True, accept=accept)
    return outs


def softmax_bwd_fp32(dy, p):
    """The chain's softmax backward in fp32 operations, in float64: dot = fmaf(dy_k, p_k, dot) over the
    classes in order, then p_k * (dy_k - dot)."""
    dy, p = dy.double(), p.double()
    dot = torch.zeros(dy.shape[:-1], dtype=torch.float64)
    for j in range(dy.shape[-1]):
        dot = fma32(dy[..., j], p[..., j], dot)
    return f32(p * f32(dy - dot[..., None]))


def usb(k, h, dtype, tols=None):
    n, ho, wo, c, dt = k["n"], k["ho"], k["wo"], k["c"], k["dt"]
    dy = host(h["dy"], dt, dtype).view(n, ho, wo, k["dyld"])[..., :c]
    p = host(h["p"], dt, dtype).view(n, ho, wo, k["yld"])[..., :c]
    if dt == BF16:
        g = bf16r(softmax_bwd_fp32(dy, p)).to(dtype)
        M = g.abs()
    else:
        g = p * (dy - (dy * p).sum(-1, keepdim=True))
        M = p.abs() * (dy.abs() + (dy * p).abs().sum(-1, keepdim=True))
    return dict(dx=Out(adjoint(g, k, dtype), adjoint(M, k, dtype), _adj_terms(k) * (c + 1), bf16=dt == BF16,
                       dropped=adjoint_less(g, k, dtype)))


_REF = {"fwd": fwd, "bwd": bwd, "usf": usf, "usa": usa, "usb": usb}


def reference(case, inputs, dtype=torch.float64, tols=None, got=None):
    """{output name: Out} of one supported case.  tols: the case's recorded tolerances (None while they are
    being recorded: no near tie of the accumulated probabilities is looked for then)."""
    assert supported(case)
    return _REF[case["kind"]](case, inputs, dtype, tols)
