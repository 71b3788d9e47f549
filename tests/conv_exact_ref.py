"""Exact integer-operand parity for the convolutions: operands, reference and conditions.

With small-integer operands every product and every partial sum of a convolution pass is an
integer below 2^24: the bf16 and fp32 MFMA, any split-K order, the fp32 slabs and the final
reductions are all exact, and the result is representable in the output type.  A kernel must
then equal the reference bit for bit whatever its summation order, and a single dropped tap,
channel chunk, pixel, tile tail or split shows as a mismatch -- no tolerance to tune.

Operands (a seeded CPU generator per case): x and dy uniform integers in [-2, 2]; the weight a
uniform sign in {-1, 0, 1} times a Bernoulli keep mask of probability
q = min(1, 768 / max(c*kh*kw, k*kh*kw)) (times ``density`` where an epilogue case needs smaller
sums); the bias uniform integers in [-3, 3].  The reference is ATen on the CPU: conv2d and its
autograd, in float64 (float32 for the largest rows: exact too under the asserted bounds).

``check_conditions`` asserts, on the reference alone, what makes the comparison valid; the tests
call it before they look at a kernel's result.  Importable without a device."""
import functools
import zlib

import torch
import torch.nn.functional as TF

LIMIT = float(1 << 24)   # integers up to 2^24 are exact in fp32
F64_WORK = 4e9           # multiply-adds of one pass above which the reference is formed in float32


class Ops:
    """Operands of one case, float64 on the CPU: x [n,c,h,w], w [k,c,kh,kh], b [k] or None,
    dy [n,k,ho,wo]; geo = (n, c, h, w, k, kh, stride, pad, dil); q = the weights' keep probability."""

    def __init__(self, geo, x, w, b, dy, q):
        self.geo, self.x, self.w, self.b, self.dy, self.q = geo, x, w, b, dy, q


class Ref:
    """Reference results (CPU, float64 or float32): y, dx, dw [k,c,kh,kh], db (None without a bias)."""

    def __init__(self, y, dx, dw, db):
        self.y, self.dx, self.dw, self.db = y, dx, dw, db


def out_hw(geo):
    n, c, h, w, k, kh, s, p, d = geo
    return (h + 2 * p - d * (kh - 1) - 1) // s + 1, (w + 2 * p - d * (kh - 1) - 1) // s + 1


def keep_prob(geo, density=1.0):
    n, c, h, w, k, kh, s, p, d = geo
    return min(1.0, 768.0 / max(c * kh * kh, k * kh * kh)) * density


def generator(*tag):
    """A CPU generator seeded from the case itself (the same on every machine and run)."""
    return torch.Generator().manual_seed(zlib.crc32(repr(tag).encode()))


def integers(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def operands(geo, bias, tag="conv", density=1.0):
    geo = tuple(geo)
    n, c, h, w, k, kh, s, p, d = geo
    g = generator(tag, geo, bias, density)
    q = keep_prob(geo, density)
    x = integers(g, (n, c, h, w), -2, 2)
    keep = (torch.rand(k, c, kh, kh, generator=g, dtype=torch.float64) < q).double()
    wt = integers(g, (k, c, kh, kh), -1, 1) * keep
    b = integers(g, (k,), -3, 3) if bias else None
    ho, wo = out_hw(geo)
    dy = integers(g, (n, k, ho, wo), -2, 2)
    return Ops(geo, x, wt, b, dy, q)


def ref_dtype(geo):
    n, c, h, w, k, kh, s, p, d = geo
    ho, wo = out_hw(geo)
    return torch.float64 if float(n) * ho * wo * k * c * kh * kh <= F64_WORK else torch.float32


def reference(ops, dtype=None):
    """conv2d and its autograd on the CPU, as tests/test_ops_gpu.py::test_conv_fwd_bwd forms them."""
    n, c, h, w, k, kh, s, p, d = ops.geo
    dtype = dtype or ref_dtype(ops.geo)
    xr = ops.x.to(dtype, copy=True).requires_grad_()  # (copies: the operands stay plain tensors)
    wr = ops.w.to(dtype, copy=True).requires_grad_()
    br = ops.b.to(dtype, copy=True).requires_grad_() if ops.b is not None else None
    y = TF.conv2d(xr, wr, br, s, p, d)
    y.backward(ops.dy.to(dtype))
    return Ref(y.detach(), xr.grad, wr.grad, br.grad if br is not None else None)


@functools.lru_cache(maxsize=2)
def case_data(geo, bias, tag="conv", density=1.0):
    """(operands, reference) of a case, formed once and shared by the tests that follow each
    other on it (both dtypes of a row; the cache stays small: the largest rows take ~0.5 GB)."""
    ops = operands(geo, bias, tag, density)
    return ops, reference(ops)


def roundtrips(t, dt):
    """t survives the conversion to dt and back unchanged."""
    return torch.equal(t.to(dt).to(t.dtype), t)


def check_operands(ops):
    """The bounds that make every partial sum exact, and non-degenerate operands."""
    n, c, h, w, k, kh, s, p, d = ops.geo
    ho, wo = out_hw(ops.geo)
    xm, dym = ops.x.abs().max().item(), ops.dy.abs().max().item()
    wa = ops.w.abs()
    # upper bounds of sum |x||w| over any receptive field (forward), of sum |dy||w| over the taps
    # that reach an input pixel (data gradient) and of sum |x||dy| over the pixels (weight gradient)
    fwd = xm * wa.sum(dim=(1, 2, 3)).max().item() + (ops.b.abs().max().item() if ops.b is not None else 0.0)
    dgr = dym * wa.sum(dim=(0, 2, 3)).max().item()
    wgr = xm * dym * n * ho * wo
    assert fwd < LIMIT and dgr < LIMIT and wgr < LIMIT, (ops.geo, fwd, dgr, wgr)
    for name, t in (("x", ops.x), ("dy", ops.dy)):
        frac = (t != 0).double().mean().item()
        assert frac >= 0.6, (ops.geo, name, frac)
        assert torch.equal(t, t.round()) and t.abs().max().item() <= 2, (ops.geo, name)
    nz = (ops.w != 0)
    assert nz.double().mean().item() >= 0.5 * ops.q, (ops.geo, "weight density", nz.double().mean().item(), ops.q)
    assert bool(nz.flatten(1).any(dim=1).all()), (ops.geo, "an output channel without a weight")
    assert bool(nz.any(dim=0).any(dim=0).all()), (ops.geo, "a filter tap without a weight")
    assert torch.equal(ops.w, ops.w.round()) and wa.max().item() <= 1, ops.geo


def check_reference(ops, ref, dts=(torch.bfloat16, torch.float32)):
    """Every reference output is representable in its output type: y and dx in the activation
    dtypes, dw and db in fp32."""
    for dt in dts:
        assert roundtrips(ref.y, dt), (ops.geo, "y", dt, ref.y.abs().max().item())
        assert roundtrips(ref.dx, dt), (ops.geo, "dx", dt, ref.dx.abs().max().item())
    assert roundtrips(ref.dw, torch.float32) and ref.dw.abs().max().item() < LIMIT, (ops.geo, "dw")
    if ref.db is not None:
        assert roundtrips(ref.db, torch.float32) and ref.db.abs().max().item() < LIMIT, (ops.geo, "db")
    for name, t in (("y", ref.y), ("dx", ref.dx), ("dw", ref.dw)):
        assert torch.equal(t, t.round()), (ops.geo, name, "not an integer")
        assert bool((t != 0).any()), (ops.geo, name, "all zero")


def check_conditions(ops, ref, dts=(torch.bfloat16, torch.float32)):
    check_operands(ops)
    check_reference(ops, ref, dts)


def check_value(t, dt, what):
    """A derived expectation (an epilogue's output, prior + reference) is representable in dt."""
    assert roundtrips(t, dt), (what, dt, t.abs().max().item())
    return t


def assert_exact(got, ref, dt, what):
    """got (a tensor of dtype dt, any device) equals ref converted to dt, element for element
    (torch.equal: +0 and -0 compare equal, a NaN equals nothing)."""
    got = got.detach().cpu()
    want = ref.detach().to(dt)
    assert got.dtype == dt, (what, got.dtype, dt)
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    g64, w64 = got.double(), want.double()
    bad = ~(g64 == w64)
    idx = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: "
                         f"got {g64[idx].item()} want {w64[idx].item()}; max |diff| "
                         f"{(g64 - w64)[bad].abs().max().item()}")


# ---- the fused inference epilogue: y = act(conv(x, w) * scale + shift + res) ---------------------
def epilogue_operands(geo, k, residual, tag="epi"):
    """scale [k] from {-1, -0.5, 0.5, 1}, shift [k] integers in [-8, 8], res integers in [-4, 4]
    (or None), float64."""
    g = generator(tag, tuple(geo), residual)
    n = geo[0]
    ho, wo = out_hw(geo)
    scale = torch.tensor([-1.0, -0.5, 0.5, 1.0], dtype=torch.float64)[torch.randint(0, 4, (k,), generator=g)]
    shift = integers(g, (k,), -8, 8)
    res = integers(g, (n, k, ho, wo), -4, 4) if residual else None
    return scale, shift, res


def epilogue_reference(conv, scale, shift, res, act):
    y = conv.double() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if res is not None:
        y = y + res
    return TF.relu(y) if act == 1 else y


# ---- the cases of tests/test_conv_exact_gpu.py (their operands are checked by test_conv_exact_cpu.py) --
def fold_geo(case):
    """(geo, residual) of a FOLD_CASES row (its bias folds into the shift, its activation is a parameter)."""
    return tuple(case[:8]) + (1,), bool(case[10])


# The register-weight direct 3x3 64 -> 64 conv takes widths with w % 64 == 0 or w % 64 > 48 only, so
# no CONV_CASES / FOLD_CASES row reaches it (their 64 -> 64 rows are 24 wide and run on the implicit
# GEMM): the smaller geometry of test_tapconv_partial_tiles stands for it, with partial column and
# row tiles.
TAP_GEO = (1, 64, 7, 56, 64, 3, 1, 1, 1)
RAGGED_GEMM_GEO = (1, 64, 13, 17, 64, 3, 1, 1, 1)
SLICE_CASE = ((1, 32, 9, 13, 32, 3, 2, 1, 1), 40, 8)  # geo, pitch, channel offset: ragged M tile

# geo, bias -- the three passes through autograd beside CONV_CASES
EXTRA_ROUTE_CASES = [
    (TAP_GEO, False),                              # tapconv forward and data gradient, partial tiles
    ((2, 64, 18, 120, 64, 3, 1, 1, 1), True),      # tapconv: 2 column tiles (the last 56 wide), rows end inside a tile
]

# geo, bias -- forward with RTSDS_ACCUMULATE
ACC_FWD_CASES = [
    (TAP_GEO, False),                              # tapconv-eligible: the flag sends it to the implicit GEMM
    ((2, 128, 8, 128, 19, 3, 1, 1, 1), False),     # hconv-eligible: the flag sends it to the implicit GEMM
    ((2, 512, 13, 21, 19, 3, 1, 4, 4), True),      # forward split-K slabs, bias, ragged M
    ((8, 256, 1, 1, 256, 1, 1, 0, 1), True),       # pooled vectors
]

# geo -- rtsds_conv2d_dgrad with accumulate = 1, one per data-gradient route
ACC_DGRAD_CASES = [
    (1, 64, 13, 17, 64, 3, 1, 2, 2),               # implicit GEMM (dilated, odd sizes)
    (2, 64, 16, 16, 128, 3, 2, 1, 1),              # stride-2 parity phases
    (2, 512, 16, 32, 512, 3, 1, 1, 1),             # split-K slabs
    TAP_GEO,                                       # tapconv
    (1, 256, 8, 64, 256, 3, 1, 1, 1),              # hconv (8 Cout chunks, N-tiled)
    (1, 128, 8, 64, 19, 3, 1, 1, 1),               # hconv-nt, 64-wide tiles, Cout 19 padded to 32
    (1, 96, 16, 32, 32, 3, 1, 1, 1),               # hconv-nt, 32-wide tiles
    (2, 512, 32, 64, 19, 1, 1, 0, 1),              # pw
    (8, 512, 1, 1, 512, 1, 1, 0, 1),               # pooled vector
    (2, 19, 1, 1, 19, 1, 1, 0, 1),                 # pooled scalar
]

# geo, bias -- rtsds_conv2d_wgrad with accumulate = 1, one per weight-gradient route
ACC_WGRAD_CASES = [
    ((2, 19, 32, 64, 64, 4, 2, 1, 1), True),       # implicit GEMM, split-K; Cin padded; dbias
    ((2, 256, 6, 100, 19, 3, 1, 1, 1), False),     # nwgrad
    ((2, 19, 16, 16, 19, 1, 1, 0, 1), True),       # narrow pointwise, two launches (also RTSDS_INPUT_PADDED)
    ((8, 256, 1, 1, 256, 1, 1, 0, 1), True),       # pooled
    ((2, 3, 32, 48, 64, 7, 2, 3, 1), False),       # superpixel view
]

# geo -- rtsds_conv2d_dgrad_act with the ReLU mask
DGRAD_ACT_CASES = [
    (1, 64, 13, 17, 64, 3, 1, 2, 2),               # implicit GEMM: mask in the epilogue
    (2, 19, 32, 64, 64, 4, 2, 1, 1),               # discriminator k4 s2: parity phases
    TAP_GEO,                                       # tapconv's own mask epilogue
    (2, 512, 16, 32, 512, 3, 1, 1, 1),             # split-K: masked by a second pass
]

# geo -- rtsds_conv2d_fwd with bn_stats
BN_STATS_CASES = [(n, c, h, w, k, 3, 1, 1, 1) for n, c, h, w, k in
                  [(2, 128, 8, 128, 19), (2, 64, 8, 64, 32), (2, 64, 6, 20, 19), (2, 256, 8, 64, 64)]] + \
                 [TAP_GEO, RAGGED_GEMM_GEO]


def epilogue_cases(fold_cases):
    """(geo, residual) of every fused-epilogue case: FOLD_CASES' geometries and the tapconv one."""
    return [fold_geo(c) for c in fold_cases] + [(TAP_GEO, True)]


def all_cases(conv_cases, fold_cases):
    """Every (geo, bias) whose operands a GPU test uses, once."""
    cases = [(tuple(c[:9]), bool(c[9])) for c in conv_cases] + EXTRA_ROUTE_CASES + ACC_FWD_CASES + ACC_WGRAD_CASES
    cases += [(g, False) for g in ACC_DGRAD_CASES + DGRAD_ACT_CASES + BN_STATS_CASES]
    cases += [(g, False) for g, _ in epilogue_cases(fold_cases)] + [(SLICE_CASE[0], False)]
    return list(dict.fromkeys(cases))
