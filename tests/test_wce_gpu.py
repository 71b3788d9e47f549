"""Class-weighted cross-entropy on the device: the fused upsample + CE (rtsds_upce_weighted_fwd),
the plain CE (rtsds_ce_weighted_*), the label statistics (rtsds_label_stats) and their way up
through train.seg_step, data parallelism and main.  The float64 reference is tests/wce_ref.py,
which tests/test_wce_cpu.py pins to torch's own fp64 chain.

Tolerances are those of the unweighted tests at the same geometries (test_ops_gpu.py): the only new
arithmetic is one fp32 multiply per term.  The identities need none: with all-ones weights every
multiply is by 1, with a uniform power of two every intermediate scales exactly, with a zero weight
a pixel contributes exact zeros -- as an ignored pixel does.  (The two scalings skip the amplitude-40
case: there the far classes' probabilities sit at the bottom of the fp32 range, where doubling and
halving are not exact; all-ones and the zero weight are checked on it too.)"""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as TF
import yaml

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import losses, optim  # noqa: E402
from rtsds_amd import main as rmain  # noqa: E402
from rtsds_amd import train as rtrain  # noqa: E402
from rtsds_amd._lib import UPCE_SET_CORRECT, lib  # noqa: E402
from rtsds_amd.callbacks import Callback  # noqa: E402
from rtsds_amd.runtime import GraphedStep  # noqa: E402

from tests import wce_ref as R  # noqa: E402
from tests.conv_cases import _close  # noqa: E402

DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.bfloat16]
GOUT = 1.5
AMP40 = 6                       # the case whose probabilities reach the subnormal range


def _dev(x, dt):
    return x.to(DEV, dt).contiguous(memory_format=torch.channels_last)


def _case(idx, dt):
    """Device heads (leaves), geometry, device target and weight of case ``idx``."""
    d = R.data(idx, dt == torch.bfloat16)
    hd = [_dev(h, dt).requires_grad_() for h in d.heads]
    geo = F.upsample_geometry(hd[0], **R.CASES[idx][4])
    assert (geo[0], geo[1]) == (d.H, d.W)
    return d, hd, geo, d.target.to(DEV), d.weight.to(DEV)


def _fused(hd, t, geo, w, gout=GOUT, want_correct=True):
    """(loss, [gradients], correct) of one fused call on fresh leaves."""
    leaves = [h.detach().clone(memory_format=torch.preserve_format).requires_grad_() for h in hd]
    correct = torch.zeros(1, dtype=torch.int64, device=DEV) if want_correct else None
    loss = F.upsample_cross_entropy(leaves, t, geo, R.IGNORE, correct, weight=w)
    loss.backward(torch.tensor(gout, device=DEV))
    return loss.detach(), [h.grad for h in leaves], None if correct is None else int(correct.item())


def _plain(x, t, w, gout=GOUT):
    leaf = x.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    loss = F.cross_entropy(leaf, t, R.IGNORE, weight=w)
    loss.backward(torch.tensor(gout, device=DEV))
    return loss.detach(), leaf.grad


# ------------------------------------------------------------------ 1. parity with fp64
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=R.IDS)
def test_fused_weighted_matches_fp64(idx, dt):
    d, hd, geo, t, w = _case(idx, dt)
    assert F.upsample_cross_entropy_supported(hd, geo, R.IGNORE, w)
    assert F.upsample_cross_entropy_supported(hd, geo, R.IGNORE)        # the plan is shared: same answer
    loss, grads, correct = _fused(hd, t, geo, w)
    ref_loss, ref_grads, up0 = R.reference(idx, dt == torch.bfloat16, GOUT)
    f32 = dt == torch.float32
    print(f"{R.IDS[idx]} {dt}: loss {float(loss)!r} fp64 {float(ref_loss)!r} rel {abs(float(loss) - float(ref_loss)) / float(ref_loss):.3e}; "
          f"grad rel max {max(float((g.double().cpu() - r).abs().max() / r.abs().max()) for g, r in zip(grads, ref_grads)):.3e}")
    _close(loss, ref_loss, torch.float32, "loss", 1e-5 if f32 else 1e-4)
    for i, (g, r) in enumerate(zip(grads, ref_grads)):
        _close(g, r, dt, f"dhead{i}", 1e-4 if f32 else 2e-2)
    # head 0's matches are unweighted (the zero-weight class counts); exact but for near-ties
    top2 = up0.topk(2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 1e-4 * up0.abs().max()).sum())
    assert abs(correct - int((up0.argmax(1) == d.target).sum())) <= near


# ------------------------------------------------------------------ 2. plain weighted CE
def _plain_data(c, bf16):
    g = torch.Generator().manual_seed(9 + c)
    x = torch.randn(2, c, 12, 20, generator=g, dtype=torch.float64) * 3
    t = torch.randint(0, c + 1, (2, 12, 20), generator=g)
    t[t == c] = R.IGNORE
    return (x.bfloat16().double() if bf16 else x), t, R.weights_for(c)


def _plain_ref(x, t, w):
    xr = x.clone().requires_grad_()
    lr = TF.cross_entropy(xr, t, weight=w.double(), ignore_index=R.IGNORE)
    lr.backward(torch.tensor(GOUT, dtype=torch.float64))
    return lr.detach(), xr.grad


@pytest.mark.parametrize("c", [19, 5, 32])
@pytest.mark.parametrize("route", ["nhwc_f32", "nhwc_bf16", "nchw_f32"])
def test_plain_weighted_ce_matches_fp64(route, c):
    bf16 = route == "nhwc_bf16"
    x, t, w = _plain_data(c, bf16)
    lr, gr = _plain_ref(x, t, w)
    if route == "nchw_f32":
        xd = x.float().to(DEV)                      # NCHW strides: the strided route
        assert xd.is_contiguous()
    else:
        xd = _dev(x, torch.bfloat16 if bf16 else torch.float32)     # the staged route
    loss, dx = _plain(xd, t.to(DEV), w.to(DEV))
    print(f"{route} c={c}: loss rel {abs(float(loss) - float(lr)) / float(lr):.3e}, dx rel "
          f"{float((dx.double().cpu() - gr).abs().max() / gr.abs().max()):.3e}")
    assert dx.stride() == xd.stride()
    _close(loss, lr, torch.float32, "ce", 1e-2 if bf16 else 1e-5)
    _close(dx, gr, xd.dtype, "dx", 3e-2 if bf16 else 1e-5)


# ------------------------------------------------------------------ 3. exact identities
def _equal_runs(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "loss", float(a[0]), float(b[0]))
    ga, gb = (a[1], b[1]) if isinstance(a[1], list) else ([a[1]], [b[1]])
    for i, (x, y) in enumerate(zip(ga, gb)):
        assert torch.equal(x, y), (what, f"gradient {i}", float((x.double() - y.double()).abs().max()))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=R.IDS)
def test_fused_identities(idx, dt):
    d, hd, geo, t, _ = _case(idx, dt)
    c = R.CASES[idx][1]
    plain = _fused(hd, t, geo, None)
    # 2 and 0.5: a missing division by the weight sum would show
    for v in (1.0,) if idx == AMP40 else (1.0, 2.0, 0.5):
        run = _fused(hd, t, geo, torch.full((c,), v, device=DEV))
        _equal_runs(run, plain, f"uniform {v}")
        assert run[2] == plain[2]
    k = c // 3
    w = torch.ones(c, device=DEV)
    w[k] = 0.0
    relabelled = torch.where(t == k, torch.full_like(t, R.IGNORE), t)
    assert int((t == k).sum()) > 0
    run, ref = _fused(hd, t, geo, w), _fused(hd, relabelled, geo, None)
    _equal_runs(run, ref, "zero weight")
    assert run[2] == plain[2]        # the zero-weight class still counts as a match


@pytest.mark.parametrize("route", ["nhwc_f32", "nhwc_bf16", "nchw_f32"])
@pytest.mark.parametrize("c", [19, 32])
def test_plain_identities(route, c):
    bf16 = route == "nhwc_bf16"
    x, t, _ = _plain_data(c, bf16)
    xd = x.float().to(DEV) if route == "nchw_f32" else _dev(x, torch.bfloat16 if bf16 else torch.float32)
    t = t.to(DEV)
    plain = _plain(xd, t, None)
    for v in (1.0, 2.0, 0.5):
        _equal_runs(_plain(xd, t, torch.full((c,), v, device=DEV)), plain, f"uniform {v}")
    k = c // 3
    w = torch.ones(c, device=DEV)
    w[k] = 0.0
    relabelled = torch.where(t == k, torch.full_like(t, R.IGNORE), t)
    _equal_runs(_plain(xd, t, w), _plain(xd, relabelled, None), "zero weight")


# ------------------------------------------------------------------ 4. fused vs the unfused weighted chain
@pytest.mark.parametrize("idx", [0, 1, 7], ids=[R.IDS[i] for i in (0, 1, 7)])
def test_fused_weighted_equals_unfused_chain_and_no_grad(idx):
    d, hd, geo, t, w = _case(idx, torch.float32)
    with torch.no_grad():
        l0 = F.upsample_cross_entropy([h.detach() for h in hd], t, geo, R.IGNORE, weight=w)
    l1, _, _ = _fused(hd, t, geo, w)
    assert torch.equal(l0, l1)
    chain = None
    for h in hd:
        l = F.cross_entropy(F.interpolate_geometry(h.detach(), geo[:4]), t, R.IGNORE, weight=w)
        chain = l if chain is None else chain + l
    _close(l0, chain, torch.float32, "loss", 1e-5)


# ------------------------------------------------------------------ 5. guarded bare entry points
GUARD, SENTINEL = 64, 0xA5


class Guarded:
    """``nbytes`` between two guards of sentinel bytes, ``offset`` bytes past a 16-B aligned base."""

    def __init__(self, nbytes, offset=0):
        self.raw = torch.full((nbytes + 2 * GUARD + offset,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.lo, self.hi = GUARD + offset, GUARD + offset + nbytes
        self.ptr = self.raw.data_ptr() + self.lo
        assert self.raw.data_ptr() % 16 == 0

    def view(self, dtype):
        return self.raw[self.lo:self.hi].view(dtype)

    def intact(self):
        return bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.hi:] == SENTINEL).all())


def _placed(flat, offset):
    """``flat`` copied ``offset`` elements past a 16-B aligned allocation; returns (keep-alive, pointer)."""
    buf = torch.zeros(flat.numel() + offset + 8, dtype=flat.dtype, device=DEV)
    buf[offset:offset + flat.numel()] = flat
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + offset * buf.element_size()


def _bare_fused(idx, dt, offset=0, nan_tail=True):
    """rtsds_upce_weighted_fwd + rtsds_upce_bwd on guarded buffers; the c weights are followed
    directly by NaNs.  Returns the raw results for bit comparisons."""
    n, c, hl, wl, resize, k = R.CASES[idx][:6]
    d = R.data(idx, dt == torch.bfloat16)
    esz = torch.empty((), dtype=dt).element_size()
    keep, ptrs = [], []
    for h in d.heads:
        b, p = _placed(h.permute(0, 2, 3, 1).reshape(-1).to(DEV, dt), offset)
        keep.append(b)
        ptrs.append(p)
    tb, tp = _placed(d.target.reshape(-1).to(DEV), offset)
    wbuf = torch.full((c + offset + 64,), float("nan") if nan_tail else 0.0, dtype=torch.float32, device=DEV)
    wbuf[offset:offset + c] = d.weight.to(DEV)
    wp = wbuf.data_ptr() + 4 * offset
    nbytes = lib.rtsds_upce_workspace(k, n, hl, wl, c, d.H, d.W, d.sh, d.sw)
    assert nbytes > 0
    ws, per_head, total, correct = Guarded(nbytes), Guarded(4 * k), Guarded(4), Guarded(8)
    dxs = [Guarded(n * hl * wl * c * esz, offset * esz) for _ in range(k)]
    st = torch.cuda.current_stream().cuda_stream
    code = F.dcode(torch.empty((), dtype=dt))
    lib.rtsds_upce_weighted_fwd(k, (ctypes.c_void_p * k)(*ptrs), tp, wp, n, hl, wl, c, d.H, d.W, d.sh, d.sw, R.IGNORE,
                                per_head.ptr, total.ptr, correct.ptr, 1 | UPCE_SET_CORRECT, code, ws.ptr, nbytes, st)
    g = torch.full((1,), GOUT, dtype=torch.float32, device=DEV)
    lib.rtsds_upce_bwd(k, g.data_ptr(), 0, (ctypes.c_void_p * k)(*[x.ptr for x in dxs]), n, hl, wl, c, d.H, d.W, d.sh, d.sw,
                       code, ws.ptr, nbytes, st)
    torch.cuda.synchronize()
    assert ws.intact() and per_head.intact() and total.intact() and correct.intact() and all(x.intact() for x in dxs)
    return (total.view(torch.float32).clone(), per_head.view(torch.float32).clone(), correct.view(torch.int64).clone(),
            [x.view(dt).clone() for x in dxs])


def _same_bits(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("idx", [0, 2, 7], ids=[R.IDS[i] for i in (0, 2, 7)])
def test_bare_fused_entry_points_stay_in_bounds_and_repeat(idx, dt):
    a = _bare_fused(idx, dt)
    assert bool(torch.isfinite(a[0]).all()) and all(bool(torch.isfinite(x.float()).all()) for x in a[3])   # no NaN weight was read
    _same_bits(a, _bare_fused(idx, dt, nan_tail=False))     # what follows the c weights does not matter
    _same_bits(a, _bare_fused(idx, dt))                     # two runs, the same bits
    _same_bits(a, _bare_fused(idx, dt, offset=1))           # bases one element off 16-B alignment
    ref_loss, ref_grads, _ = R.reference(idx, dt == torch.bfloat16, GOUT)
    _close(a[0].reshape(()), ref_loss, torch.float32, "loss", 1e-5 if dt == torch.float32 else 1e-4)
    n, c, hl, wl = R.CASES[idx][:4]
    for x, r in zip(a[3], ref_grads):
        _close(x.view(n, hl, wl, c).permute(0, 3, 1, 2), r, dt, "dhead", 1e-4 if dt == torch.float32 else 2e-2)


@pytest.mark.parametrize("route", ["nhwc_f32", "nhwc_bf16", "nchw_f32"])
def test_bare_plain_entry_points_never_read_past_the_weights(route):
    c, n, h, w = 19, 2, 12, 20
    bf16 = route == "nhwc_bf16"
    dt = torch.bfloat16 if bf16 else torch.float32
    x, t, wt = _plain_data(c, bf16)
    nchw = route == "nchw_f32"
    flat = (x if nchw else x.permute(0, 2, 3, 1)).reshape(-1).to(DEV, dt).contiguous()
    sn, sc, shw = (c * h * w, h * w, 1) if nchw else (h * w * c, 1, c)
    td = t.to(DEV)
    out = []
    for tail in (float("nan"), 0.0):
        wbuf = torch.full((c + 64,), tail, dtype=torch.float32, device=DEV)
        wbuf[:c] = wt.to(DEV)
        nbytes = lib.rtsds_ce_workspace()
        ws, loss, dx = Guarded(nbytes), Guarded(4), Guarded(flat.numel() * flat.element_size())
        st = torch.cuda.current_stream().cuda_stream
        lib.rtsds_ce_weighted_fwd(flat.data_ptr(), sn, sc, shw, td.data_ptr(), wbuf.data_ptr(), loss.ptr, n, h * w, c, R.IGNORE,
                                  F.dcode(flat), ws.ptr, nbytes, st)
        g = torch.full((1,), GOUT, dtype=torch.float32, device=DEV)
        lib.rtsds_ce_weighted_bwd(flat.data_ptr(), sn, sc, shw, td.data_ptr(), wbuf.data_ptr(), g.data_ptr(), ws.ptr + 4 * 2048,
                                  dx.ptr, n, h * w, c, R.IGNORE, F.dcode(flat), st)
        torch.cuda.synchronize()
        assert ws.intact() and loss.intact() and dx.intact()
        out.append((loss.view(torch.float32).clone(), dx.view(dt).clone()))
    assert bool(torch.isfinite(out[0][0]).all()) and bool(torch.isfinite(out[0][1].float()).all())
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    lr, _ = _plain_ref(x, t, wt)
    _close(out[0][0].reshape(()), lr, torch.float32, "ce", 1e-2 if bf16 else 1e-5)


# ------------------------------------------------------------------ 6. label statistics
def _stats(labels, c, ignore, count=None, support=None):
    count = torch.zeros(c, dtype=torch.int64, device=DEV) if count is None else count
    support = torch.zeros(c, dtype=torch.int64, device=DEV) if support is None else support
    F.label_stats(labels.to(DEV), c, ignore, count, support)
    return count, support


def _check_stats(labels, c, ignore):
    count, support = _stats(labels, c, ignore)
    rc, rs = R.label_stats(labels.numpy(), c, ignore)
    assert count.cpu().numpy().tolist() == rc.tolist()
    assert support.cpu().numpy().tolist() == rs.tolist()
    return count, support


def test_label_stats_exact():
    g = torch.Generator().manual_seed(4)
    lab = torch.randint(0, 20, (3, 37, 53), generator=g)          # 19 = the ignore value
    lab[torch.rand(lab.shape, generator=g) < 0.05] = 255
    lab[0, 3, 4] = -1
    lab[1, 30, 50] = 19 + 5
    lab[2][lab[2] == 7] = 8                                      # class 7 is missing from the last image
    _check_stats(lab, 19, 19)
    # the guarded workspace and outputs of the bare entry point stay intact
    nbytes = lib.rtsds_label_stats_workspace(3, 19)
    ws, count, support = Guarded(nbytes), Guarded(19 * 8), Guarded(19 * 8)
    count.view(torch.int64).zero_()
    support.view(torch.int64).zero_()
    ld = lab.to(DEV)
    lib.rtsds_label_stats(ld.data_ptr(), 3, 37, 53, 19, 19, count.ptr, support.ptr, ws.ptr, nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ws.intact() and count.intact() and support.intact()
    rc, rs = R.label_stats(lab.numpy(), 19, 19)
    assert count.view(torch.int64).cpu().tolist() == rc.tolist() and support.view(torch.int64).cpu().tolist() == rs.tolist()


def test_label_stats_single_pixel_and_32_classes():
    for v in (0, 18, 19, 255):
        _check_stats(torch.full((1, 1, 1), v, dtype=torch.int64), 19, 19)
    g = torch.Generator().manual_seed(6)
    _check_stats(torch.randint(-2, 36, (2, 41, 67), generator=g), 32, 33)


def test_label_stats_last_pixel_and_accumulation():
    lab = torch.zeros(2, 37, 53, dtype=torch.int64)
    lab[1, 36, 52] = 11                                          # the only pixel of class 11: the very last
    count, support = _check_stats(lab, 19, 19)
    assert int(count[11]) == 1 and int(support[11]) == 37 * 53
    g = torch.Generator().manual_seed(8)
    more = torch.randint(0, 20, (3, 16, 24), generator=g)
    _stats(more, 19, 19, count, support)                         # a second call adds
    rc0, rs0 = R.label_stats(lab.numpy(), 19, 19)
    rc1, rs1 = R.label_stats(more.numpy(), 19, 19)
    assert count.cpu().tolist() == (rc0 + rc1).tolist() and support.cpu().tolist() == (rs0 + rs1).tolist()


# ------------------------------------------------------------------ 7. train.seg_step
def _fro(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _noise_bounded(ours, ref32, ref64, what, floor=1e-3, factor=2.0):
    """tests/test_models_gpu.py's rule: per tensor, ||ours - exact|| <= factor * the fp32 oracle's own
    worst relative distance from the fp64 oracle + floor (Frobenius, relative to ||exact||); tensors
    whose exact value is ~0 are skipped."""
    keys = [k for k, g in ref64.items() if g is not None and g.double().norm() >= 1e-8]
    e_ref = {k: _fro(ref32[k], ref64[k]) for k in keys}
    e_ours = {k: _fro(ours[k], ref64[k]) for k in keys}
    bound = factor * max(e_ref.values()) + floor
    worst = max(keys, key=lambda k: e_ours[k])
    assert e_ours[worst] <= bound, (what, worst, e_ours[worst], bound)
    return worst, e_ours[worst], max(e_ref.values())


def _load(model, seed=1):
    from oracle.weights import recipe_state_dict
    sd = model.state_dict()
    model.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed))
    return model


def test_seg_step_weighted_takes_the_fused_path_and_matches_the_oracle(monkeypatch):
    from oracle import models as om
    from oracle import steps as osteps
    from oracle.weights import synthetic_images, synthetic_labels
    from rtsds_amd.models.bisenet.build_bisenet import BiSeNet
    x, y = synthetic_images(2, 64, 128, seed=42), synthetic_labels(2, 64, 128, seed=43)
    w = R.weights_for(19)
    ref = {}
    for dt in (torch.float64, torch.float32):
        net = _load(om.BiSeNet(19, "resnet18")).to(dt).train()
        out = osteps.seg_step(net, torch.optim.Adam(net.parameters(), lr=1e-4),
                              torch.nn.CrossEntropyLoss(weight=w.to(dt), ignore_index=19), x.to(dt), y)
        ref[dt] = (out["loss"], {k: p.grad for k, p in net.named_parameters() if p.grad is not None})

    seen = []
    real = F.upsample_cross_entropy

    def spy(*a, **k):
        seen.append(k.get("weight"))
        return real(*a, **k)
    monkeypatch.setattr(F, "upsample_cross_entropy", spy)
    crit = losses.CrossEntropyLoss(weight=w, ignore_index=19).to(DEV)
    xd, yd = x.to(DEV), y.to(DEV)

    def run(graphed):
        with rtsds_amd.precision(torch.float32):
            net = _load(BiSeNet(19, "resnet18")).to(DEV).train()
            opt = optim.Adam(net.parameters(), lr=1e-4)

            def core():
                return rtrain.seg_step(net, crit, opt, xd, yd)
            first = core()
            first = (first[0].clone(), first[1].clone())
            grads1 = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
            step = GraphedStep(core, [opt], warmup=0) if graphed else core
            loss, correct = step()
            torch.cuda.synchronize()
            return (first, grads1, loss.clone(), correct.clone(), {k: v.detach().clone() for k, v in net.state_dict().items()},
                    {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
    eager = run(False)
    assert seen and all(s is crit.weight for s in seen)           # the fused path, with the weight
    (loss1, _), grads1 = eager[0], eager[1]
    l32 = ref[torch.float32][0]
    print(f"weighted seg step: loss {float(loss1)!r}, oracle fp32 {l32!r}, fp64 {ref[torch.float64][0]!r}")
    assert abs(float(loss1) - l32) < 1e-4 * l32
    # (torchvision's unused fc keeps the zeros of zero_grad here and no gradient in the oracle)
    extra = set(grads1) - set(ref[torch.float64][1])
    assert set(ref[torch.float64][1]) <= set(grads1) and all(not grads1[k].any() for k in extra), extra
    print("weighted seg step grads worst:", _noise_bounded(grads1, ref[torch.float32][1], ref[torch.float64][1], "seg grad"))
    graphed = run(True)
    assert torch.equal(eager[2], graphed[2]) and torch.equal(eager[3], graphed[3])
    for k in eager[4]:
        assert torch.equal(eager[4][k], graphed[4][k]), k
    for k in eager[5]:
        assert torch.equal(eager[5][k], graphed[5][k]), k


# ------------------------------------------------------------------ 8. two ranks on one GPU
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_data():
    """A gathered batch of four images, two heads through one shared per-class scale; the first
    shard's labels are half ignored and biased to the heavy classes, so the shards' weight sums differ."""
    g = torch.Generator().manual_seed(17)
    base = [torch.randn(4, 19, 8, 16, generator=g) * 2 for _ in range(2)]
    scale = 0.5 + torch.rand(1, 19, 1, 1, generator=g)
    t = torch.randint(0, 19, (4, 64, 128), generator=g)
    t[:2] = t[:2] % 5
    t[:2][torch.rand(t[:2].shape, generator=g) < 0.5] = R.IGNORE
    return base, scale, t, R.weights_for(19)


def _dp_losses(base, scale, t, w):
    s = scale.to(DEV).requires_grad_()
    heads = [(b.to(DEV) * s).contiguous(memory_format=torch.channels_last) for b in base]
    for h in heads:
        h.retain_grad()
    geo = F.upsample_geometry(heads[0], scale_factor=8)
    loss = F.upsample_cross_entropy(heads, t.to(DEV), geo, R.IGNORE, weight=w.to(DEV))
    loss.backward()
    return loss.detach(), s.grad, [h.grad for h in heads]


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dist.init_process_group("gloo")
    try:
        base, scale, t, w = _dp_data()
        sl = slice(2 * rank, 2 * rank + 2)
        loss, gs, gh = _dp_losses([b[sl] for b in base], scale, t[sl], w)
        both = torch.cat([loss.reshape(1).double(), gs.reshape(-1).double()])
        dist.all_reduce(both)                                   # the ranks' contributions SUM
        torch.save({"heads": [g.cpu() for g in gh], "local_loss": float(loss)}, f"{out}.{rank}")
        if rank == 0:
            torch.save({"loss": float(both[0]), "gscale": both[1:].cpu()}, out)
    finally:
        dist.destroy_process_group()


def test_two_ranks_sum_to_the_gathered_batch(tmp_path):
    out = str(tmp_path / "dp.pt")
    ctx = mp.get_context("spawn")
    port = _port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    got = torch.load(out, weights_only=True)
    parts = [torch.load(f"{out}.{r}", weights_only=True) for r in range(2)]
    base, scale, t, w = _dp_data()
    sums = [float(w[t[2 * r:2 * r + 2][t[2 * r:2 * r + 2] != R.IGNORE]].sum()) for r in range(2)]
    assert abs(sums[0] - sums[1]) > 0.2 * max(sums)              # the premise: unequal weight sums
    loss, gs, gh = _dp_losses(base, scale, t, w)
    lv = float(loss)
    print(f"two ranks: loss {got['loss']!r} (locals {[p['local_loss'] for p in parts]}) vs gathered {lv!r}")
    assert abs(got["loss"] - lv) <= 1e-5 * abs(lv), (got["loss"], lv)       # test_dp_gpu.py's loss tolerance
    _close(got["gscale"], gs.reshape(-1), torch.float32, "shared-scale gradient", 1e-5)
    for h in range(2):
        _close(torch.cat([parts[0]["heads"][h], parts[1]["heads"][h]]), gh[h], torch.float32, f"dhead{h}", 1e-5)


# ------------------------------------------------------------------ 9. main
def test_main_installs_inverse_log_weights_from_the_synthetic_labels(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))
    cfg["precision"] = "fp32"
    cfg["data"]["cityscapes"].update(image_size="64, 128", batch_size=2)
    cfg["data"]["gta5_modified"].update(image_size="64, 128", batch_size=2)
    cfg["data"]["synthetic_batches"] = 2
    cfg["training"]["segmentation"].update(epochs=1)
    cfg["model"]["bisenet"]["criterion"]["weight"] = "inverse_log"
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    seen = {"losses": [], "crit": None, "loader": None}
    real_train = rmain.train

    class Log(Callback):
        def on_batch_end(self, batch, logs=None):
            seen["losses"].append(logs["train_loss"])

    def wrapped(**kw):
        seen["crit"], seen["loader"] = kw["criterion"], kw["train_loader"]
        kw["callbacks"] = list(kw["callbacks"]) + [Log()]
        return real_train(**kw)
    monkeypatch.setattr(rmain, "train", wrapped)
    before = rtsds_amd.compute_dtype()
    try:
        rmain.main(["--config", str(p), "--model", "bisenet"])
    finally:
        rtsds_amd.set_compute_dtype(before)
    labels = np.concatenate([y.numpy().reshape(-1) for _, y in seen["loader"]])
    count = np.bincount(labels[labels != 19], minlength=19)[:19]
    want = losses.class_weights(count, mode="inverse_log")
    got = seen["crit"].weight
    assert got.is_cuda and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), np.float32(want))
    assert len(seen["losses"]) == 2 and all(np.isfinite(v) and v > 0 for v in seen["losses"])
