"""Exact integer-operand parity of every convolution route and epilogue (GPU only).

tests/test_ops_gpu.py compares the convolutions with a tolerance of 3e-2 * max|ref| in bf16 mode,
loose enough to miss a lost tile tail in the gradients that reduce over pixels.  Here the operands
are small integers (tests/conv_exact_ref.py): every product and partial sum is an integer below
2^24, so the MFMA, any split-K order, the fp32 slabs and the reductions are exact and each result
must equal the ATen CPU reference bit for bit (torch.equal) -- forward, data gradient, weight and
bias gradient, the fused inference epilogue, the accumulate flags, the deferred split reduce, the
ReLU-masked data gradient and the data gradient's BatchNorm-backward partials.  The only
tolerances left are those of the forward BatchNorm partials' mean and variance (2e-4, the
project's fp32 tolerance).  Every test asserts the conditions on the reference first.

A library built with the weight-gradient GEMM's ragged final K-tile skipped passes the bf16 runs
of test_conv_fwd_bwd on both persistent rows (8x128x67x131, 24x64x161x97) and fails here on them.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd._lib import ACCUMULATE, INPUT_PADDED, lib  # noqa: E402
from rtsds_amd.functional import _conv_desc, _P  # noqa: E402
from rtsds_amd.nn import _shadow  # noqa: E402
from rtsds_amd.runtime import stream, workspace  # noqa: E402
from tests import conv_exact_ref as E  # noqa: E402
from tests.conv_cases import CONV_CASES, FOLD_CASES  # noqa: E402

DEV = "cuda"
CL = torch.channels_last
BF16, F32 = torch.bfloat16, torch.float32
DTS = (BF16, F32)
NAN = float("nan")


def _dev(t, dt):
    return t.to(dt).to(DEV).contiguous(memory_format=CL)


def _f32(t):
    return None if t is None else t.float().to(DEV).contiguous()


def _desc(xd, geo):
    n, c, h, w, k, kh, s, p, d = geo
    return _conv_desc(xd, k, kh, kh, (s, s), (p, p), (d, d))


def _id(v):
    if isinstance(v, tuple):
        return "x".join(str(int(i)) for i in v)
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    return str(v)


def _setup(geo, bias, dt):
    """Operands and reference of a case (conditions asserted), x / w / dy on the device in dt, the
    descriptor."""
    ops, ref = E.case_data(tuple(geo), bool(bias))
    E.check_conditions(ops, ref, (dt,))
    xd, wd, dyd = _dev(ops.x, dt), _dev(ops.w, dt), _dev(ops.dy, dt)
    return ops, ref, xd, wd, dyd, _desc(xd, geo)


def _nhwc_out(shape, dt, fill=NAN):
    return torch.full(tuple(shape), fill, dtype=dt, device=DEV).contiguous(memory_format=CL)


def _kernel_dw(t):
    """[k, c, kh, kw] -> the kernels' [k][kh][kw][c]."""
    return t.permute(0, 2, 3, 1).contiguous()


# ---- a. every route, all three passes --------------------------------------------------------
ROUTE_CASES = [(tuple(c[:9]), c[9]) for c in CONV_CASES] + E.EXTRA_ROUTE_CASES


@pytest.mark.parametrize("geo,bias,dt", [(g, b, dt) for g, b in ROUTE_CASES for dt in DTS], ids=_id)
def test_conv_fwd_bwd_exact(geo, bias, dt):
    """F.conv2d and its backward, driven as test_conv_fwd_bwd drives them: y, dx, dw and db equal the
    reference bit for bit on every row of CONV_CASES -- the implicit GEMM (plain, split-K,
    persistent, stride-2 phases), hconv / hconv-nt / nwgrad, imgconv and the superpixel view, pw /
    pwn and the pooled-vector kernels -- and on two tapconv geometries, which no CONV_CASES row
    reaches (see conv_exact_ref.TAP_GEO)."""
    n, c, h, w, k, kh, s, p, d = geo
    ops, ref = E.case_data(geo, bias)
    E.check_conditions(ops, ref, (dt,))
    xd = _dev(ops.x, dt).requires_grad_()
    wp = torch.nn.Parameter(ops.w.float().to(DEV).contiguous(memory_format=CL))
    bp = torch.nn.Parameter(ops.b.float().to(DEV)) if bias else None
    y = F.conv2d(xd, wp, bp, _shadow(wp, dt), (s, s), (p, p), (d, d), 0)
    y.backward(_dev(ops.dy, dt))
    torch.cuda.synchronize()
    E.assert_exact(y, ref.y, dt, "y")
    E.assert_exact(xd.grad, ref.dx, dt, "dx")
    E.assert_exact(wp.grad, ref.dw, F32, "dw")
    if bias:
        E.assert_exact(bp.grad, ref.db, F32, "db")


# ---- b. the fused inference epilogue on each forward route -----------------------------------
@pytest.mark.parametrize("geo,residual,act,dt", [(g, r, a, dt) for g, r in E.epilogue_cases(FOLD_CASES)
                                                 for a in (0, 1) for dt in DTS], ids=_id)
def test_conv_fwd_bn_exact(geo, residual, act, dt):
    """rtsds_conv2d_fwd_bn through the C ABI with chosen scale / shift: y = act(conv * scale +
    shift [+ res]), scale in {-1, -0.5, 0.5, 1}, integer shift and residual, act NONE and RELU, on
    FOLD_CASES' geometries -- superpixel / imgconv, the implicit GEMM with and without residual
    (64x64 and 128x128 tiles, scalar epilogue for 19 outputs), both pooled kernels, both halo
    tilings with residual -- and tapconv with residual."""
    ops, ref, xd, wd, _, d = _setup(geo, False, dt)
    n, k = geo[0], geo[4]
    scale, shift, res = E.epilogue_operands(geo, k, residual)
    want = E.check_value(E.epilogue_reference(ref.y, scale, shift, res, act), dt, "epilogue")
    y = _nhwc_out(ref.y.shape, dt)
    ws = workspace(lib.rtsds_conv2d_fwd_workspace(ctypes.byref(d)), xd.device)
    resd = _dev(res, dt) if residual else None
    sc, sh = _f32(scale), _f32(shift)
    assert lib.rtsds_conv2d_fwd_bn(ctypes.byref(d), _P(xd), _P(wd), _P(sc), _P(sh), _P(resd), _P(y), act, _P(ws),
                                   ws.numel(), stream()) == 0
    torch.cuda.synchronize()
    E.assert_exact(y, want, dt, "y")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dt", DTS, ids=_id)
def test_conv_fwd_bn_slice_exact(dt, act):
    """rtsds_conv2d_fwd_bn_ld: the row-pitched epilogue with a ragged M tile (35 output pixels)
    writes the exact result into channels [8, 40) of a 40-channel buffer and leaves channels
    [0, 8) untouched."""
    geo, ld, off = E.SLICE_CASE
    ops, ref, xd, wd, _, d = _setup(geo, False, dt)
    n, k = geo[0], geo[4]
    ho, wo = E.out_hw(geo)
    scale, shift, _ = E.epilogue_operands(geo, k, False)
    want = E.check_value(E.epilogue_reference(ref.y, scale, shift, None, act), dt, "epilogue")
    buf = torch.full((n, ho, wo, ld), 7.0, dtype=dt, device=DEV)
    ws = workspace(lib.rtsds_conv2d_fwd_workspace(ctypes.byref(d)), xd.device)
    sc, sh = _f32(scale), _f32(shift)
    assert lib.rtsds_conv2d_fwd_bn_ld(ctypes.byref(d), _P(xd), _P(wd), _P(sc), _P(sh),
                                      buf.data_ptr() + off * buf.element_size(), ld, act, _P(ws), ws.numel(),
                                      stream()) == 0
    torch.cuda.synchronize()
    E.assert_exact(buf[..., off:off + k].permute(0, 3, 1, 2), want, dt, "slice")
    assert torch.equal(buf[..., :off], torch.full_like(buf[..., :off], 7.0))
    assert off + k == ld


# ---- c. accumulate flags ---------------------------------------------------------------------
@pytest.mark.parametrize("geo,bias,dt", [(g, b, dt) for g, b in E.ACC_FWD_CASES for dt in DTS], ids=_id)
def test_fwd_accumulate_exact(geo, bias, dt):
    """rtsds_conv2d_fwd with RTSDS_ACCUMULATE: y = prior + conv + bias exactly, on a tapconv- and
    a hconv-eligible shape (the flag sends both to the implicit GEMM), the forward split-K shape of
    test_fwd_split_k_accumulate (bias and prior added by the split reduce) and a pooled vector."""
    ops, ref, xd, wd, _, d = _setup(geo, bias, dt)
    y0 = E.integers(E.generator("prior-y", geo), ref.y.shape, -4, 4)
    want = E.check_value(y0 + ref.y.double(), dt, "prior + y")
    y = _dev(y0, dt)
    ws = workspace(lib.rtsds_conv2d_fwd_workspace(ctypes.byref(d)), xd.device)
    bd = _f32(ops.b)
    assert lib.rtsds_conv2d_fwd(ctypes.byref(d), _P(xd), _P(wd), _P(bd), _P(y), ACCUMULATE, None, _P(ws), ws.numel(),
                                stream()) == 0
    torch.cuda.synchronize()
    E.assert_exact(y, want, dt, "y accumulate")


@pytest.mark.parametrize("geo,dt", [(g, dt) for g in E.ACC_DGRAD_CASES for dt in DTS], ids=_id)
def test_dgrad_accumulate_exact(geo, dt):
    """rtsds_conv2d_dgrad, plain and with accumulate = 1 (dx = prior + dgrad exactly), one shape
    per data-gradient route (bf16): implicit GEMM, stride-2 phases, split-K, tapconv, hconv,
    hconv-nt at both tile widths, pw, pooled vector and pooled scalar; in fp32 the same shapes on
    the routes that mode has."""
    ops, ref, xd, wd, dyd, d = _setup(geo, False, dt)
    dx0 = E.integers(E.generator("prior-dx", geo), ref.dx.shape, -4, 4)
    want = E.check_value(dx0 + ref.dx.double(), dt, "prior + dx")
    dx, fresh = _dev(dx0, dt), _nhwc_out(ref.dx.shape, dt)
    ws = workspace(lib.rtsds_conv2d_dgrad_workspace(ctypes.byref(d)), xd.device)
    for out, acc in ((dx, 1), (fresh, 0)):
        assert lib.rtsds_conv2d_dgrad(ctypes.byref(d), _P(dyd), _P(wd), _P(out), acc, _P(ws), ws.numel(), stream()) == 0
    torch.cuda.synchronize()
    E.assert_exact(fresh, ref.dx, dt, "dx")
    E.assert_exact(dx, want, dt, "dx accumulate")


@pytest.mark.parametrize("geo,bias,dt", [(g, b, dt) for g, b in E.ACC_WGRAD_CASES for dt in DTS], ids=_id)
def test_wgrad_accumulate_exact(geo, bias, dt):
    """rtsds_conv2d_wgrad, plain and with accumulate = 1 (dw / db = prior + gradient exactly), one
    shape per weight-gradient route (bf16): split-K implicit GEMM with padded Cin, nwgrad, the
    narrow pointwise two-launch route, pooled, the superpixel view; where the route gathers x with
    a padded channel pitch, also from an image stored with that pitch (RTSDS_INPUT_PADDED)."""
    n, c, h, w, k, kh, s, p, dil = geo
    ops, ref, xd, wd, dyd, d = _setup(geo, bias, dt)
    g = E.generator("prior-dw", geo)
    dw_ref = _kernel_dw(ref.dw.double())
    dw0 = E.integers(g, dw_ref.shape, -4, 4)
    db0 = E.integers(g, (k,), -4, 4)
    want_w = E.check_value(dw0 + dw_ref, F32, "prior + dw")
    want_b = E.check_value(db0 + ref.db.double(), F32, "prior + db") if bias else None
    ws = workspace(lib.rtsds_conv2d_wgrad_workspace(ctypes.byref(d)), xd.device)

    def run(x, flags, prior):
        dw = _f32(dw0) if prior else torch.full(dw_ref.shape, NAN, dtype=F32, device=DEV)
        db = (_f32(db0) if prior else torch.full((k,), NAN, dtype=F32, device=DEV)) if bias else None
        assert lib.rtsds_conv2d_wgrad(ctypes.byref(d), _P(x), _P(dyd), _P(dw), _P(db), flags, _P(ws), ws.numel(),
                                      stream()) == 0
        torch.cuda.synchronize()
        return dw, db

    variants = [("", xd, 0)]
    pitch = lib.rtsds_conv2d_input_pitch(ctypes.byref(d))
    if pitch != c:
        xp = torch.nn.functional.pad(xd.permute(0, 2, 3, 1), (0, pitch - c)).contiguous()  # NHWC, padded pitch
        variants.append((" (padded x)", xp, INPUT_PADDED))
    for name, x, flag in variants:
        dw, db = run(x, flag, False)
        E.assert_exact(dw, dw_ref, F32, "dw" + name)
        if bias:
            E.assert_exact(db, ref.db, F32, "db" + name)
        dw, db = run(x, 1 | flag, True)
        E.assert_exact(dw, want_w, F32, "dw accumulate" + name)
        if bias:
            E.assert_exact(db, want_b, F32, "db accumulate" + name)


@pytest.mark.parametrize("geo,bias,dt", [(g, b, dt) for g, b in E.ACC_WGRAD_CASES for dt in DTS], ids=_id)
def test_wgrad_deferred_reduce_exact(geo, bias, dt):
    """rtsds_conv2d_wgrad_deferred + rtsds_split_reduce_many, as the training backward drives the
    weight gradients into the optimizer's arena: with accumulate = 1, dw / db = prior + gradient
    exactly once the pending reduction (where the route leaves one) has run; before it, a deferred
    dw still holds the prior."""
    from rtsds_amd._lib import SplitReduceDesc
    k = geo[4]
    ops, ref, xd, wd, dyd, d = _setup(geo, bias, dt)
    g = E.generator("prior-dw", geo)
    dw_ref = _kernel_dw(ref.dw.double())
    dw0 = E.integers(g, dw_ref.shape, -4, 4)
    db0 = E.integers(g, (k,), -4, 4)
    want_w = E.check_value(dw0 + dw_ref, F32, "prior + dw")
    dw, db = _f32(dw0), (_f32(db0) if bias else None)
    ws = workspace(lib.rtsds_conv2d_wgrad_workspace(ctypes.byref(d)), xd.device)
    pend = SplitReduceDesc()
    assert lib.rtsds_conv2d_wgrad_deferred(ctypes.byref(d), _P(xd), _P(dyd), _P(dw), _P(db), 1, _P(ws), ws.numel(),
                                           ctypes.byref(pend), stream()) == 0
    if pend.nv > 0:
        torch.cuda.synchronize()
        E.assert_exact(dw, dw0, F32, "dw before the deferred reduce")
        assert pend.dw == dw.data_ptr() and pend.accumulate == 1
        assert lib.rtsds_split_reduce_many(1, (SplitReduceDesc * 1)(pend), stream()) == 0
    torch.cuda.synchronize()
    E.assert_exact(dw, want_w, F32, "dw accumulate")
    if bias:
        E.assert_exact(db, E.check_value(db0 + ref.db.double(), F32, "prior + db"), F32, "db accumulate")


# ---- d. data gradient with the ReLU mask -----------------------------------------------------
@pytest.mark.parametrize("geo,dt", [(g, dt) for g in E.DGRAD_ACT_CASES for dt in DTS], ids=_id)
def test_dgrad_relu_mask_exact(geo, dt):
    """rtsds_conv2d_dgrad_act with act 1 and an integer x_act with zeros and negatives in it:
    dx = dgrad * (x_act > 0) exactly -- the mask in the GEMM epilogue, in the stride-2 phases of
    the discriminator's k4 s2 conv, in tapconv's epilogue, and as a second pass after split-K."""
    ops, ref, xd, wd, dyd, d = _setup(geo, False, dt)
    xa = E.integers(E.generator("x_act", geo), ref.dx.shape, -2, 2)
    assert 0.1 < (xa > 0).double().mean().item() < 0.9 and bool((xa == 0).any())
    want = ref.dx.double() * (xa > 0)
    dx = _nhwc_out(ref.dx.shape, dt)
    ws = workspace(lib.rtsds_conv2d_dgrad_workspace(ctypes.byref(d)), xd.device)
    xad = _dev(xa, dt)
    assert lib.rtsds_conv2d_dgrad_act(ctypes.byref(d), _P(dyd), _P(wd), _P(dx), _P(xad), 1, _P(ws), ws.numel(),
                                      stream()) == 0
    torch.cuda.synchronize()
    E.assert_exact(dx, want, dt, "dx masked")


@pytest.mark.parametrize("geo", [E.RAGGED_GEMM_GEO, (2, 64, 16, 24, 64, 3, 1, 1, 1), E.TAP_GEO], ids=_id)
def test_dgrad_bn_backward_partials_exact(geo):
    """rtsds_conv2d_dgrad_bnstats (bf16; the GEMM epilogue with a ragged and a full last M tile,
    and tapconv's): dx stays bit-equal, and with integer BatchNorm operands (gamma in {1, 2}, beta
    and mean in [-1, 1], invstd 1) the per-tile partials (sum g, sum g (bn_x - mean)),
    g = dx * (gamma (bn_x - mean) + beta > 0), are integers below 2^24: summed over the tiles they
    equal the reference exactly."""
    dt = BF16
    n, c, h, w = geo[:4]
    ops, ref, xd, wd, dyd, d = _setup(geo, False, dt)
    tiles = lib.rtsds_conv2d_dgrad_bnstats_tiles(ctypes.byref(d))
    assert tiles > 0
    g = E.generator("bn-bwd", geo)
    bx = E.integers(g, ref.dx.shape, -2, 2)
    gamma, beta, mean = E.integers(g, (c,), 1, 2), E.integers(g, (c,), -1, 1), E.integers(g, (c,), -1, 1)
    col = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    gg = ref.dx.double() * ((col(gamma) * (bx - col(mean)) + col(beta)) > 0)
    want = torch.stack([gg.sum(dim=(0, 2, 3)), (gg * (bx - col(mean))).sum(dim=(0, 2, 3))], 1)
    assert (gg.abs() * (bx - col(mean)).abs()).sum(dim=(0, 2, 3)).max().item() < E.LIMIT
    guard = 1024
    part = torch.full((c * tiles * 2 + guard,), -7.0, dtype=F32, device=DEV)
    dx = _nhwc_out(ref.dx.shape, dt)
    bxd, gd, bd, md, iv = _dev(bx, dt), _f32(gamma), _f32(beta), _f32(mean), torch.ones(c, dtype=F32, device=DEV)
    ws = workspace(lib.rtsds_conv2d_dgrad_workspace(ctypes.byref(d)), xd.device)
    assert lib.rtsds_conv2d_dgrad_bnstats(ctypes.byref(d), _P(dyd), _P(wd), _P(dx), _P(bxd), _P(gd), _P(bd), _P(md),
                                          _P(iv), 1, _P(part), _P(ws), ws.numel(), stream()) == 0
    torch.cuda.synchronize()
    E.assert_exact(dx, ref.dx, dt, "dx")
    assert bool((part[c * tiles * 2:] == -7.0).all()), "wrote past the partials"
    got = part[:c * tiles * 2].double().cpu().view(c, tiles, 2)
    assert torch.equal(got, got.round())
    E.assert_exact(got.sum(1), want, torch.float64, "sum g, sum g (x - mean)")


# ---- e. conv-epilogue BatchNorm partials -----------------------------------------------------
@pytest.mark.parametrize("geo,dt", [(g, dt) for g in E.BN_STATS_CASES for dt in DTS], ids=_id)
def test_conv_bn_stats_partials(geo, dt):
    """rtsds_conv2d_fwd with bn_stats on test_conv_bn_stats_epilogue's shapes (hconv and the GEMM
    epilogue), tapconv and a ragged GEMM shape: the [k][tiles][count, mean, M2, 0] partials,
    combined on the host in float64 with the parallel-variance formula, count N*Ho*Wo per channel
    exactly and give the mean within 2e-4 of max|y| and the biased variance within 2e-4 of the
    variance; nothing is written past the k * tiles * 4 floats; y stays bit-equal."""
    ops, ref, xd, wd, _, d = _setup(geo, False, dt)
    n, k = geo[0], geo[4]
    ho, wo = E.out_hw(geo)
    tiles = lib.rtsds_conv2d_fwd_stats_tiles(ctypes.byref(d))
    assert tiles > 0
    guard = 1024
    stats = torch.full((k * tiles * 4 + guard,), -7.0, dtype=F32, device=DEV)
    y = _nhwc_out(ref.y.shape, dt)
    ws = workspace(lib.rtsds_conv2d_fwd_workspace(ctypes.byref(d)), xd.device)
    assert lib.rtsds_conv2d_fwd(ctypes.byref(d), _P(xd), _P(wd), None, _P(y), 0, _P(stats), _P(ws), ws.numel(),
                                stream()) == 0
    torch.cuda.synchronize()
    E.assert_exact(y, ref.y, dt, "y")
    assert bool((stats[k * tiles * 4:] == -7.0).all()), "wrote past the partials"
    s = stats[:k * tiles * 4].double().cpu().view(k, tiles, 4)
    cnt, mu, m2 = s[:, :, 0], s[:, :, 1], s[:, :, 2]
    tot = cnt.sum(1)
    assert torch.equal(tot, torch.full_like(tot, float(n * ho * wo))), tot
    assert bool((cnt >= 0).all()) and torch.equal(cnt, cnt.round())
    mean = (cnt * mu).sum(1) / tot
    var = (m2 + cnt * (mu - mean[:, None]) ** 2).sum(1) / tot
    yr = ref.y.double()
    mean_ref, var_ref = yr.mean(dim=(0, 2, 3)), yr.var(dim=(0, 2, 3), unbiased=False)
    assert bool((var_ref > 0).all())
    merr = (mean - mean_ref).abs().max().item()
    verr = ((var - var_ref).abs() / var_ref).max().item()
    print(f"bn partials {geo} {dt}: tiles {tiles}, mean err {merr:.3e} (max|y| {yr.abs().max().item():.0f}), "
          f"var rel err {verr:.3e}")
    assert merr <= 2e-4 * yr.abs().max().item()
    assert verr <= 2e-4
