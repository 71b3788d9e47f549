"""The premises of the route-reference suites (tests/test_{bn,chan,resize}_route_ref_gpu.py), on the CPU:
every case and output has a recorded tolerance; the references (tests/*_route_ref.py) are torch's where torch
has the operation; no case excludes more than the cap allows; and the comparison (tests/route_compare.py)
accepts the float32 evaluation of a reference as a kernel's output but rejects it once one element is off
by four allowances, two neighbouring pixels are swapped, the last pixel is left unwritten or one term of a
reduction is missing."""
import math

import pytest
import torch
import torch.nn.functional as TF

from tests import bn_bits_cases, bn_route_ref, chan_bits_cases, chan_route_ref, resize_bits_cases, resize_route_ref
from tests import route_compare as RC
from tests.bn_bits_cases import BF16, F32, NONE, UNWRITTEN

UNITS = {"bn": (bn_bits_cases, bn_route_ref), "chan": (chan_bits_cases, chan_route_ref),
         "resize": (resize_bits_cases, resize_route_ref)}
TOL = RC.load_tol()
ALL = [(u, c) for u, (cases, _) in UNITS.items() for c in cases.CASES]
ALL_IDS = [f"{u}-{UNITS[u][0].case_id(c)}" for u, c in ALL]
F64 = torch.float64


def _supported(ref, case):
    return not hasattr(ref, "supported") or ref.supported(case)


def test_the_tolerance_file_covers_the_case_tables():
    assert sorted(TOL) == sorted(UNITS)
    for unit, (cases, _) in UNITS.items():
        assert sorted(TOL[unit]) == sorted(cases.IDS)


@pytest.mark.parametrize("unit,case", ALL, ids=ALL_IDS)
def test_every_output_has_a_tolerance_and_the_exclusions_keep_to_the_cap(unit, case):
    cases, ref = UNITS[unit]
    tols = TOL[unit][cases.case_id(case)]
    if not _supported(ref, case):
        assert tols == {"y": "unwritten"}
        return
    outs = ref.reference(case, cases.host_inputs(case), F64, tols)
    assert sorted(outs) == sorted(tols)
    for name, o in outs.items():
        if o.exact:
            assert tols[name] == RC.EXACT
        else:
            assert isinstance(tols[name], float) and math.isfinite(tols[name]) and tols[name] > 0
        assert o.excluded() <= RC.MAX_EXCLUDED, f"{name}: {o.excluded():.3e} of the elements excluded"
    if "_doubtful_masks" in outs:      # no ReLU / Leaky mask recomputed from x is within an fp32 error of zero
        assert int(outs["_doubtful_masks"].val) == 0


# ------------------------------------------------------------------ the references are torch's
def _close(a, b, what):
    a, b = a.double().flatten(), b.double().flatten()
    assert a.shape == b.shape, what
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), f"{what}: off by {err:.3e}"


@pytest.mark.parametrize("act,res", [(bn_bits_cases.NONE, False), (bn_bits_cases.RELU, True), (bn_bits_cases.SIGMOID, False)])
def test_batch_norm_is_torchs(act, res):
    rows, c = 40, 24
    k = dict(kind="fwd", rows=rows, c=c, dt=F32, act=act, res=res, training=1, nrb=0)
    h = bn_bits_cases.host_inputs(k)
    f = bn_route_ref.reference(k, h, F64)
    x = torch.from_numpy(h["x"]).double().view(rows, c).requires_grad_()
    gamma, beta = torch.from_numpy(h["gamma"]).double().requires_grad_(), torch.from_numpy(h["beta"]).double().requires_grad_()
    rm, rv = torch.from_numpy(h["rmean"]).double().clone(), torch.from_numpy(h["rvar"]).double().clone()
    y = TF.batch_norm(x, rm, rv, gamma, beta, True, bn_route_ref.MOM, bn_route_ref.EPSF)
    r = torch.from_numpy(h["res"]).double().view(rows, c).requires_grad_() if res else None
    if res:
        y = y + r
    y = {bn_bits_cases.NONE: y, bn_bits_cases.RELU: y.relu(), bn_bits_cases.SIGMOID: y.sigmoid()}[act]
    _close(f["y"].val, y.detach(), "y")
    _close(f["running_mean"].val, rm, "running_mean")
    _close(f["running_var"].val, rv, "running_var")
    _close(f["save_mean"].val, x.detach().mean(0), "save_mean")
    _close(f["save_invstd"].val, 1 / torch.sqrt(x.detach().var(0, unbiased=False) + bn_route_ref.EPSF), "save_invstd")
    # the backward with the forward's own statistics and output (consistent inputs) is autograd's
    kb = dict(kind="bwd", rows=rows, c=c, dt=F32, act=act, y=True, dx=True, dres=res, training=1, acc=0)
    dy = torch.from_numpy(bn_bits_cases.pattern(rows * c, 4) / 4).double().view(rows, c)
    y.backward(dy)
    hb = dict(x=x.detach().numpy(), dy=dy.numpy(), y=y.detach().numpy(), gamma=gamma.detach().numpy(), beta=beta.detach().numpy(),
              mean=f["save_mean"].val.numpy(), invstd=f["save_invstd"].val.numpy())
    b = bn_route_ref.bwd(kb, hb, F64)
    _close(b["dx"].val, x.grad, "dx")
    _close(b["dgamma"].val, gamma.grad, "dgamma")
    _close(b["dbeta"].val, beta.grad, "dbeta")
    if res:
        _close(b["dres"].val, r.grad, "dres")
    if act != bn_bits_cases.SIGMOID:   # the mask recomputed from x gives the same
        b2 = bn_route_ref.bwd(dict(kb, y=False, dres=False), dict(hb, y=None), F64) if not res else None
        if b2:
            _close(b2["dx"].val, x.grad, "dx from x")


def test_eval_mode_batch_norm_is_torchs():
    k = dict(kind="fwd", rows=40, c=24, dt=F32, act=NONE, res=False, training=0, nrb=0)
    h = bn_bits_cases.host_inputs(k)
    f = bn_route_ref.reference(k, h, F64)
    d = {n: torch.from_numpy(h[n]).double() for n in ("x", "gamma", "beta", "rmean", "rvar")}
    y = TF.batch_norm(d["x"].view(40, 24), d["rmean"], d["rvar"], d["gamma"], d["beta"], False, 0.1, bn_route_ref.EPSF)
    _close(f["y"].val, y, "y")


def test_max_pool_is_torchs():
    k = bn_bits_cases.CASES[-1]
    assert k["kind"] == "pool"
    n, hh, ww, c, p = k["n"], k["h"], k["w"], k["c"], k["p"]
    ho, wo, rows, _ = bn_bits_cases.pool_geo(k)
    f = bn_route_ref.reference(k, bn_bits_cases.host_inputs(k), F64)
    act = RC.bf16r(f["_act"].val).view(n, hh, ww, c).permute(0, 3, 1, 2)
    y, flat = TF.max_pool2d(act, 3, 2, p, return_indices=True)
    ih, iw = flat // ww, flat % ww
    oh, ow = torch.arange(ho).view(1, 1, ho, 1), torch.arange(wo).view(1, 1, 1, wo)
    tap = (ih - (oh * 2 - p)) * 3 + (iw - (ow * 2 - p))
    assert torch.equal(f["idx"].val, tap.permute(0, 2, 3, 1))
    _close(RC.bf16r(f["y"].val), y.permute(0, 2, 3, 1), "y")


def _chan(kind, **kw):
    k = dict(kind=kind, dt=F32, **kw)
    return k, chan_bits_cases.host_inputs(k)


@pytest.mark.parametrize("lay", ["nhwc", "nchw", "slice"])
def test_softmax_and_cross_entropy_are_torchs(lay):
    n, hw, c = 2, 150, 19
    k, h = _chan("smf", n=n, hw=hw, c=c, lay=lay, ld=0, off=0)
    x = chan_route_ref._logits(h["x"], k, F32, F64).clone().requires_grad_()     # [n][hw][c]
    y = torch.softmax(x, -1)
    _close(chan_route_ref.reference(k, h, F64)["y"].val, y.detach(), "softmax")
    kb, hb = _chan("smb", n=n, hw=hw, c=c, lay=lay, ld=0, off=0)
    yb = torch.from_numpy(hb["y"]).double().view(n, hw, c).requires_grad_()
    dy = torch.from_numpy(hb["dy"]).double().view(n, hw, c)
    # dx = y (dy - sum dy y) is the vector-Jacobian product of softmax at any y
    want = yb.detach() * (dy - (dy * yb.detach()).sum(-1, keepdim=True))
    got = chan_route_ref.reference(kb, hb, F64)["dx"]
    sel = ~got.fixed.flatten() if got.fixed is not None else slice(None)
    if lay == "nchw":
        want = want.permute(0, 2, 1)
    _close(got.val.flatten()[sel], want.flatten(), "softmax backward")
    y.backward(dy)
    _close(x.grad, y.detach() * (dy - (dy * y.detach()).sum(-1, keepdim=True)), "autograd of softmax")
    if lay == "slice":
        return
    kc, hc = _chan("ce", n=n, hw=hw, c=c, lay=lay, tgt="idx")
    xc = chan_route_ref._logits(hc["x"], kc, F32, F64).clone().requires_grad_()
    loss = TF.cross_entropy(xc.reshape(-1, c), torch.from_numpy(hc["tgt"]), ignore_index=chan_bits_cases.IGNORE)
    (2 * loss).backward()
    f = chan_route_ref.reference(kc, hc, F64)
    _close(f["loss"].val, loss.detach(), "cross entropy")
    _close(f["dx"].val, xc.grad.permute(0, 2, 1) if lay == "nchw" else xc.grad, "cross entropy gradient")
    assert float(f["ws"].val[0]) == float((torch.from_numpy(hc["tgt"]) != chan_bits_cases.IGNORE).sum())
    _close(f["loss_finish"].val, f["ws"].val[1] / 123, "finish")


def test_bce_argmax_and_bincount_are_torchs():
    k, h = _chan("bce", n=300)
    x, t = torch.from_numpy(h["x"]).double().requires_grad_(), torch.from_numpy(h["t"]).double()
    loss = TF.binary_cross_entropy_with_logits(x, t)
    (2 * loss).backward()
    f = chan_route_ref.reference(k, h, F64)
    _close(f["loss"].val, loss.detach(), "bce")
    _close(f["dx"].val, x.grad, "bce gradient")
    for lay in ("nhwc", "nchw"):
        k, h = _chan("am", n=4, hw=1000, c=3, lay=lay, null="")
        xx = torch.from_numpy(h["x"]).double()
        want = (xx.view(4, 3, 1000).argmax(1) if lay == "nchw" else xx.view(4, 1000, 3).argmax(2)).flatten()
        f = chan_route_ref.reference(k, h, F64)
        assert torch.equal(f["out"].val, want)
        assert int(f["correct"].val) == 5 + int((want == torch.from_numpy(h["tgt"])).sum())
    k, h = _chan("conf", total=300, nc=19)
    lab, pred = torch.from_numpy(h["label"]), torch.from_numpy(h["pred"])
    ok = (lab >= 0) & (lab < 19)
    want = torch.from_numpy(h["hist0"]) + torch.bincount(19 * lab[ok] + pred[ok], minlength=361)
    assert torch.equal(chan_route_ref.reference(k, h, F64)["hist"].val, want)


def test_nan_rows_of_the_argmax_reference():
    k, h = _chan("am", n=2, hw=150, c=19, lay="nhwc", null="")
    out = chan_route_ref.reference(k, h, F64)["out"].val
    p = torch.arange(300)
    assert bool((out[p % 11 == 2] == 0).all()) and bool((out[p % 11 == 5] == 7).all()) and bool((out[p % 11 == 8] == 5).all())


# scales that are exact in fp32, so that torch's float64 scale is the driver's
@pytest.mark.parametrize("src,dst", [((4, 5), (8, 10)), ((3, 5), (12, 20)), ((8, 12), (4, 6)), ((2, 128), (2, 8192))])
def test_bilinear_resize_and_its_adjoint_are_torchs(src, dst):
    k = dict(kind="fwd", n=2, c=3, hi=src[0], wi=src[1], ho=dst[0], wo=dst[1], dt=F32, ld=0, off=0, s=0)
    h = resize_bits_cases.host_inputs(k)
    x = torch.from_numpy(h["x"]).double().view(2, src[0], src[1], 3).permute(0, 3, 1, 2).clone().requires_grad_()
    y = TF.interpolate(x, size=dst, mode="bilinear", align_corners=False)
    _close(resize_route_ref.reference(k, h, F64)["y"].val, y.detach().permute(0, 2, 3, 1), "resize")
    kb = dict(k, kind="bwd")
    hb = resize_bits_cases.host_inputs(kb)
    dy = torch.from_numpy(hb["dy"]).double().view(2, dst[0], dst[1], 3)
    y.backward(dy.permute(0, 3, 1, 2))
    _close(resize_route_ref.reference(kb, hb, F64)["dx"].val, x.grad.permute(0, 2, 3, 1), "adjoint")


def test_the_fp32_statement_of_the_resized_logits_is_the_resize():
    k = dict(kind="usf", n=2, c=19, hi=3, wi=40, ho=5, wo=300, dt=BF16, yld=32)
    h = resize_bits_cases.host_inputs(k)
    x = RC.host(h["x"], BF16, F64).view(2, 3, 40, 19)
    exact, fp32 = resize_route_ref.resize(x, k, F64), resize_route_ref.resize_fp32(x, k)
    assert float((exact - fp32).abs().max()) <= 8 * 2.0 ** -23 * 8 + 2.0 ** -24 * 40 * 16   # blend + source index roundings


# ------------------------------------------------------------------ the comparison notices what it must
# one case of each kind: (unit, index into its table, the pixel tensor, channels per pixel there)
def _first(cases, kind, **kw):
    return next(c for c in cases.CASES if c["kind"] == kind and all(c[a] == b for a, b in kw.items()))


SENS = [("bn", _first(bn_bits_cases, "fwd", rows=2000, act=1, res=False, nrb=0, training=1), "y", "save_mean"),
        ("bn", _first(bn_bits_cases, "bwd", rows=2000, act=1, y=False, acc=0, training=1), "dx", "dbeta"),
        ("bn", _first(bn_bits_cases, "part", nrb=5, acc=0), "dx", "dbeta"),
        ("bn", _first(bn_bits_cases, "pool"), "dx", "dbeta"),
        ("chan", _first(chan_bits_cases, "smf", dt=BF16, c=19, lay="nhwc", ld=32), "y", "y"),
        ("chan", _first(chan_bits_cases, "smb", dt=F32, c=19, lay="slice"), "dx", "dx"),
        ("chan", _first(chan_bits_cases, "ce", dt=BF16, lay="nhwc", tgt="idx", hw=150), "dx", "loss"),
        ("chan", _first(chan_bits_cases, "am", dt=BF16, lay="nchw", null="", hw=150), None, None),
        ("chan", _first(chan_bits_cases, "bce", n=300), "dx", "loss"),
        ("chan", _first(chan_bits_cases, "conf"), None, None),
        ("chan", _first(chan_bits_cases, "gapf", dt=BF16, hw=2088, c=19), None, "y"),
        ("chan", _first(chan_bits_cases, "gapb", dt=BF16, c=19, acc=1), "dx", None),
        ("chan", _first(chan_bits_cases, "csf", dt=BF16, mode=1), "y", None),
        ("chan", _first(chan_bits_cases, "csb", dt=F32, mode=1, outs="da", c=19), None, "da"),
        ("chan", _first(chan_bits_cases, "ffm", dt=BF16), "out", "out"),
        ("resize", _first(resize_bits_cases, "fwd", dt=BF16, c=67), "y", None),
        ("resize", _first(resize_bits_cases, "bwd", dt=F32, c=19, ho=97), "dx", "dx"),
        ("resize", _first(resize_bits_cases, "usf", dt=BF16, c=19, yld=24), "y", "y"),
        ("resize", _first(resize_bits_cases, "usa", dt=BF16, c=19, flip=1, acc=1, pred=1, wo=301), "acc", "acc"),
        ("resize", _first(resize_bits_cases, "usb", dt=BF16, c=19, dyld=24), "dx", "dx")]


def _stored(o):
    """A reference output as the kernel would have stored it."""
    v = o.val.contiguous().clone()
    if o.exact:
        return v
    return v.to(torch.bfloat16) if o.bf16 else v.float()


def _rejects(cid, ref, got, tols):
    with pytest.raises(AssertionError, match=cid.replace("(", r"\(").replace(")", r"\)")[:20]):
        RC.check_case(cid, ref, got, tols)
    return True


@pytest.mark.parametrize("unit,case,pix,summed", SENS, ids=[f"{u}-{c['kind']}" for u, c, _, _ in SENS])
def test_the_comparison_accepts_the_float32_evaluation_and_rejects_what_it_must(unit, case, pix, summed):
    cases, ref = UNITS[unit]
    cid = cases.case_id(case)
    tols, h = TOL[unit][cid], cases.host_inputs(case)
    r64, r32 = ref.reference(case, h, F64, tols), ref.reference(case, h, torch.float32, tols)
    public = [n for n, o in r64.items() if not o.private]
    good = {n: _stored(r32[n]) for n in public}
    # outputs of which the reference states a part (the cross-entropy workspace) arrive whole
    for n in public:
        if r64[n].sel is not None:
            whole = torch.full((int(r64[n].sel.max()) + 8,), float("nan"))
            whole[r64[n].sel] = good[n].float()
            good[n] = whole
    ratios = RC.check_case(cid, r64, good, tols)
    assert max(ratios.values()) <= 1.0
    for n in public:
        if r64[n].exact:                     # an integer output: one element off by one is noticed
            bad = dict(good)
            bad[n] = good[n].clone()
            bad[n].view(-1)[bad[n].numel() // 2] += 1
            assert _rejects(cid, r64, bad, tols)
    if pix is not None:
        o = r64[pix]
        free = ~o.fixed.flatten() if o.fixed is not None else torch.ones(o.val.numel(), dtype=torch.bool)
        want = o.val.double().flatten()
        allow = tols[pix] + (RC.BF16_OUT * want.abs() if o.bf16 else 0.0)
        # one element moved by four times what it is allowed
        i = int(free.nonzero()[free.sum() // 2])
        bad = dict(good)
        bad[pix] = good[pix].clone().double()
        bad[pix].view(-1)[i] = want[i] + 4 * float(allow[i] if o.bf16 else allow)
        assert _rejects(cid, r64, bad, tols)
        # two neighbouring pixels swapped (the pair that differs most)
        cpp = o.val.shape[-1] if o.val.dim() > 1 else 1
        rows = good[pix].clone().view(-1, cpp)
        j = int((want.view(-1, cpp)[1:] - want.view(-1, cpp)[:-1]).abs().amax(1).argmax())
        rows[[j, j + 1]] = rows[[j + 1, j]]
        bad[pix] = rows
        assert _rejects(cid, r64, bad, tols)
        # the last pixel left as the driver filled it
        rows = good[pix].clone().view(-1, cpp)
        rows[-1, free.view(-1, cpp)[-1]] = UNWRITTEN
        bad[pix] = rows
        assert _rejects(cid, r64, bad, tols)
    if summed is not None:                   # one term of a reduction dropped
        bad = dict(good)
        bad[summed] = _stored(RC.Out(r32[summed].dropped, bf16=r32[summed].bf16))
        assert _rejects(cid, r64, bad, tols)
