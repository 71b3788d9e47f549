"""The Adam step fused with the split-K weight-gradient reductions (rtsds_adam_step_slabs,
functional.FUSE_REDUCE_ADAM) against what it replaces, bit for bit.

Op level: the fused entry against rtsds_split_reduce_many + rtsds_adam_step_dev on synthetic slabs,
with guards around every buffer.  Model level: BiSeNet-R18 seg_steps with the switch off and on,
eagerly and as hipGraph replays, and the fallbacks (da_step, a forced unsupported return, gradients
read before the step, zero_grad after a fallback step).  Everything is compared with torch.equal.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import losses, optim  # noqa: E402
from rtsds_amd import train as rtrain  # noqa: E402
from rtsds_amd._lib import SplitReduceDesc, lib, load  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402
from rtsds_amd.models.domain_shift.adversarial.model import TinyDomainDiscriminator  # noqa: E402
from rtsds_amd.runtime import GraphedStep, stream  # noqa: E402

DEV = "cuda"
GUARD = 256        # elements of sentinel on both sides of every buffer
SENT = 12345.0
KEEP = optim.SLAB_KEEP_GRAD


# ----------------------------------------------------------------------------- op level
def _slab(rows, cv, cp, splits, acc=False, keep=False):
    return dict(rows=rows, cv=cv, cp=cp, splits=splits, acc=acc, keep=keep)


# One arena run, segments of 64 floats as optim._Arena lays them out.  ("plain", n): a parameter whose
# gradient is in the arena.  Slabs: nv = rows * cv float4 outputs, cp the slab's channel pitch.
#   nv 1 / 63 / 64 / 65 / 128 / 1024 / 27 / 8 / 8; splits 1, 3, 4, 5, 33, 100 (fewer than the four groups,
#   not a multiple of 4, more than one 32-stride pass), 40, 2, 7; padded pitch (cp != 4 cv) in four of them;
#   a hole at the very start and one at the very end; nv 64 (256 floats) is followed directly by a
#   1-element plain parameter and that by the next hole; the nv 128 and nv 1024 holes are adjacent;
#   two holes hold an earlier contribution; two keep their gradient; a plain gap longer than two blocks.
LAYOUT = [
    _slab(1, 1, 4, 1),
    _slab(9, 7, 32, 3),
    _slab(8, 8, 32, 4),
    ("plain", 1),
    _slab(5, 13, 64, 5, acc=True),
    ("plain", 16),
    _slab(16, 8, 32, 33),
    _slab(64, 16, 64, 100),
    ("plain", 9000),
    _slab(27, 1, 4, 40, keep=True),
    _slab(4, 2, 8, 2, acc=True, keep=True),
    ("plain", 64),
    _slab(2, 4, 16, 7),
]


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
    body = buf[GUARD:GUARD + n]
    body.copy_(fill.to(dtype))
    return buf, body


def _guards_ok(buf, n):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all())


def _build(layout, seed):
    """The arena run of ``layout``: (n, holes [(offset, spec, slab tensor)], generator)."""
    g = torch.Generator().manual_seed(seed)
    off, holes = 0, []
    for seg in layout:
        if isinstance(seg, tuple):
            numel = seg[1]
        else:
            numel = 4 * seg["rows"] * seg["cv"]
            slab = torch.randn(seg["splits"], seg["rows"] * seg["cp"], generator=g).to(DEV)
            holes.append((off, seg, slab))
        end = off + numel
        off = (end + 63) // 64 * 64
    return end, holes, g  # the run ends with its last parameter, not with the padding


def _descs(holes, gbody, flags):
    arr = (SplitReduceDesc * len(holes))()
    for k, (off, seg, slab) in enumerate(holes):
        arr[k].slab, arr[k].dw = slab.data_ptr(), gbody.data_ptr() + 4 * off
        arr[k].slab_stride, arr[k].nv = slab.shape[1], seg["rows"] * seg["cv"]
        arr[k].cv, arr[k].cp, arr[k].splits = seg["cv"], seg["cp"], seg["splits"]
        arr[k].accumulate = flags(seg)
    return arr


def _state(n, g):
    p = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01
    grad = torch.randn(n, generator=g)
    return p, m, v, grad


HYPER = [1e-3, 1.0 - 0.9 ** 3, (1.0 - 0.999 ** 3) ** 0.5]


def _op_case(layout, wd, seed=0):
    n, holes, g = _build(layout, seed)
    assert n <= 200_000
    p0, m0, v0, g0 = _state(n, g)
    hyper = torch.tensor(HYPER, dtype=torch.float32, device=DEV)
    out = {}
    for fused in (False, True):
        bufs = {k: _guarded(n, torch.float32, t) for k, t in (("p", p0), ("m", m0), ("v", v0), ("g", g0))}
        bufs["s"] = _guarded(n, torch.bfloat16, torch.zeros(n))
        gb = bufs["g"][1]
        for off, seg, _ in holes:
            span = gb[off:off + 4 * seg["rows"] * seg["cv"]]
            if not seg["acc"]:
                # no earlier contribution: the reduce adds onto the zeros of zero_grad; the fused
                # launch must not read the range at all, so it gets NaN there
                span.fill_(float("nan") if fused else 0.0)
        gin = gb.clone()
        ptrs = [bufs[k][1].data_ptr() for k in ("p", "g", "m", "v", "s")]
        if fused:
            arr = _descs(holes, gb, lambda s: (1 if s["acc"] else 0) | (KEEP if s["keep"] else 0))
            rc = load().rtsds_adam_step_slabs(*ptrs, n, hyper.data_ptr(), 0.9, 0.999, 1e-8, wd, 1.0, 0, len(holes), arr, 0,
                                              stream())
            assert rc == 0
        else:
            lib.rtsds_split_reduce_many(len(holes), _descs(holes, gb, lambda s: 1), stream())
            lib.rtsds_adam_step_dev(*ptrs, n, hyper.data_ptr(), 0.9, 0.999, 1e-8, wd, 1.0, 0, stream())
        torch.cuda.synchronize()
        for k, (buf, _) in bufs.items():
            assert _guards_ok(buf, n), (fused, k)
        out[fused] = {k: body.clone() for k, (_, body) in bufs.items()}
        out[fused]["gin"] = gin
    ref, got = out[False], out[True]
    for k in ("p", "m", "v", "s"):
        assert torch.equal(ref[k], got[k]), (k, int((ref[k] != got[k]).sum()))
    assert not torch.equal(ref["p"], p0.to(DEV))
    # the gradient arena: a kept hole holds the reduced gradient, everything else is as it was
    want = got["gin"].clone()
    for off, seg, _ in holes:
        if seg["keep"]:
            sl = slice(off, off + 4 * seg["rows"] * seg["cv"])
            want[sl] = ref["g"][sl]
    assert torch.equal(want.view(torch.int32), got["g"].view(torch.int32))  # (bit patterns: the NaN fills too)


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_fused_entry_equals_reduce_then_adam(wd):
    _op_case(LAYOUT, wd)


@pytest.mark.parametrize("tail", [1, 5, 7])
def test_run_ending_in_a_plain_parameter_that_is_no_whole_vector(tail):
    _op_case(LAYOUT + [("plain", tail)], 1e-4, seed=1)


def test_no_descriptor_is_the_plain_step():
    _op_case([("plain", 5000), ("plain", 3)], 1e-4, seed=2)


def test_more_descriptors_than_the_cap_is_unsupported_and_touches_nothing():
    layout = [_slab(1, 1, 4, 2) for _ in range(57)]
    n, holes, g = _build(layout, 3)
    p0, m0, v0, g0 = _state(n, g)
    hyper = torch.tensor(HYPER, dtype=torch.float32, device=DEV)
    bufs = {k: _guarded(n, torch.float32, t) for k, t in (("p", p0), ("m", m0), ("v", v0), ("g", g0))}
    bufs["s"] = _guarded(n, torch.bfloat16, torch.zeros(n))
    before = {k: buf.clone() for k, (buf, _) in bufs.items()}
    ptrs = [bufs[k][1].data_ptr() for k in ("p", "g", "m", "v", "s")]
    arr = _descs(holes, bufs["g"][1], lambda s: 0)
    fn = load().rtsds_adam_step_slabs
    assert fn(*ptrs, n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1.0, 0, 57, arr, 0, stream()) == 2
    assert fn(*ptrs, n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1.0, 0, 3, arr, 2, stream()) == 2   # a lower cap
    assert fn(*ptrs, n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1.0, 1, 3, arr, 0, stream()) == 2   # a bf16 wire gradient
    # malformed lists are refused before any launch as well: unsorted, overlapping, outside the run
    swapped = (SplitReduceDesc * 2)(arr[1], arr[0])
    assert fn(*ptrs, n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1.0, 0, 2, swapped, 0, stream()) == 1
    twice = (SplitReduceDesc * 2)(arr[0], arr[0])
    assert fn(*ptrs, n, hyper.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1.0, 0, 2, twice, 0, stream()) == 1
    assert fn(*ptrs, 64, hyper.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1.0, 0, 2, arr, 0, stream()) == 1
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert torch.equal(buf, before[k]), k


def test_zero_ranges():
    n = 3 * 4096 + 70
    buf, body = _guarded(n, torch.float32, torch.ones(n))
    rng = [(0, 1), (3, 3), (5, 64), (64, 4096 + 64 + 3), (2 * 4096 + 1, n)]
    lo = (ctypes.c_long * len(rng))(*[r[0] for r in rng])
    hi = (ctypes.c_long * len(rng))(*[r[1] for r in rng])
    lib.rtsds_zero_ranges(body.data_ptr(), len(rng), lo, hi, stream())
    torch.cuda.synchronize()
    want = torch.ones(n)
    for a, b in rng:
        want[a:b] = 0
    assert torch.equal(body.cpu(), want) and _guards_ok(buf, n)


# ----------------------------------------------------------------------------- model level
def _batch(seed=21):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 3, 128, 256, generator=g).to(DEV)
    xt = torch.randn(2, 3, 128, 256, generator=g).to(DEV)
    y = torch.randint(0, 20, (2, 128, 256), generator=g).to(DEV)
    return x, xt, y


def _snapshot(net, opts):
    st = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for oi, o in enumerate(opts):
        for ai, a in enumerate(o.arenas()):
            st.update({f"o{oi}.{ai}.p": a.flat.clone(), f"o{oi}.{ai}.exp_avg": a.m.clone(),
                       f"o{oi}.{ai}.exp_avg_sq": a.v.clone(), f"o{oi}.{ai}.shadow": a.shadow.clone()})
    return st


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


class _Spy:
    """Counts optim.Adam._launch_slabs calls by outcome."""

    def __init__(self, monkeypatch):
        self.taken, self.refused = 0, 0
        self.targets = {}  # (arena, parameter index) -> keep, of the fused launches
        real = optim.Adam._launch_slabs

        def spy(opt, *a):
            ok = real(opt, *a)
            self.taken += bool(ok)
            self.refused += not ok
            if ok:
                self.targets.update({it[3]._rt_arena: it[4] for it in a[-1]})
            return ok
        monkeypatch.setattr(optim.Adam, "_launch_slabs", spy)


def _seg_run(fuse, graphed, steps=3, between=None):
    """``steps`` seg_steps of BiSeNet-R18 (2x3x128x256, bf16) with FUSE_REDUCE_ADAM = fuse: the
    losses, the accuracy counts and the state after.  ``between(i, opt)``: called before step i."""
    x, _, y = _batch()
    ce = losses.CrossEntropyLoss(ignore_index=19)
    old = F.FUSE_REDUCE_ADAM
    F.FUSE_REDUCE_ADAM = fuse
    try:
        with rtsds_amd.precision(torch.bfloat16):
            torch.manual_seed(4)
            net = BiSeNet(19, "resnet18").to(DEV).train()
            opt = optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-4)
            core = lambda: rtrain.seg_step(net, ce, opt, x, y)  # noqa: E731
            step = GraphedStep(core, [opt], warmup=1) if graphed else core  # (graphed: one more, eager, step first)
            outs = []
            for i in range(steps):
                if between is not None:
                    between(i, opt)
                loss, correct = step()
                outs.append((loss.clone(), correct.clone()))
            torch.cuda.synchronize()
            return outs, _snapshot(net, [opt]), opt
    finally:
        F.FUSE_REDUCE_ADAM = old


_REF = {}


def _ref(graphed):
    if graphed not in _REF:
        outs, st, _ = _seg_run(False, graphed)
        _REF[graphed] = (outs, st)
    return _REF[graphed]


def _outs_equal(a, b):
    assert len(a) == len(b)
    for (la, ca), (lb, cb) in zip(a, b):
        assert torch.equal(la, lb) and torch.equal(ca, cb)


@pytest.mark.parametrize("graphed", [False, True])
def test_bisenet_fused_reduce_adam_bit_identical(graphed, monkeypatch):
    assert F.FUSE_REDUCE_ADAM
    ref_outs, ref_st = _ref(graphed)
    spy = _Spy(monkeypatch)
    outs, st, opt = _seg_run(True, graphed)
    # every eager step, and the warm-up step and each capture of the graphed run, took the fused launch
    assert spy.taken >= (2 if graphed else 3) and spy.refused == 0
    _outs_equal(ref_outs, outs)
    _same(ref_st, st)
    # what the fused step consumed never reached the arena, the two image convs' kept gradients did
    assert sorted(spy.targets.values()).count(True) == 2 and len(spy.targets) >= 20
    for (a, i), keep in spy.targets.items():
        grad = a.gflat[a.offsets[i]:a.offsets[i] + a.params[i].numel()]
        assert a.dirty[i] == keep and bool(grad.any()) == keep, (i, keep)


def test_forced_unsupported_return_falls_back_with_the_same_bits(monkeypatch):
    ref_outs, ref_st = _ref(False)
    spy = _Spy(monkeypatch)
    monkeypatch.setattr(optim.Adam, "SLAB_MAX_DESCS", 1)  # the hole list is over the cap: RTSDS_ERR_UNSUPPORTED
    outs, st, _ = _seg_run(True, False)
    assert spy.taken == 0 and spy.refused >= 3
    _outs_equal(ref_outs, outs)
    _same(ref_st, st)


def test_zero_grad_after_a_fallback_step_leaves_no_stale_gradient(monkeypatch):
    ref_outs, ref_st = _ref(False)
    spy = _Spy(monkeypatch)
    seen = []

    def between(i, opt):
        optim.Adam.SLAB_MAX_DESCS = 1 if i == 0 else 0  # step 0 falls back, steps 1 and 2 are fused
        if i == 1:
            # the fallback wrote every weight gradient into the arena; the zero_grad that opens
            # step 1 must clear them although the fused steps never dirty those ranges
            arenas = opt.arenas()
            assert any(a.gflat.any() for a in arenas)
            opt.zero_grad()
            seen.append(all(not a.gflat.any() for a in arenas))
    try:
        outs, st, _ = _seg_run(True, False, between=between)
    finally:
        optim.Adam.SLAB_MAX_DESCS = 0
    assert seen == [True]
    assert spy.refused >= 1 and spy.taken >= 2
    _outs_equal(ref_outs, outs)
    _same(ref_st, st)


def test_gradients_read_before_the_step_are_the_parents(monkeypatch):
    x, _, y = _batch()
    ce = losses.CrossEntropyLoss(ignore_index=19)
    res = {}
    for fuse in (False, True):
        monkeypatch.setattr(F, "FUSE_REDUCE_ADAM", fuse)
        with rtsds_amd.precision(torch.bfloat16):
            torch.manual_seed(4)
            net = BiSeNet(19, "resnet18").to(DEV).train()
            opt = optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-4)
            opt.zero_grad()
            o, a1, a2 = net(x)
            loss = ce(o, y) + ce(a1, y) + ce(a2, y)
            rtrain._fuse_reduce(opt)
            loss.backward()
            if fuse:
                assert opt._pending  # handed over, not reduced
            opt.materialize_grads()
            assert not opt._pending
            grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
            opt.step()
            torch.cuda.synchronize()
            res[fuse] = (grads, _snapshot(net, [opt]))
    assert any(bool(v.any()) for v in res[True][0].values())
    _same(res[False][0], res[True][0])
    _same(res[False][1], res[True][1])


def test_da_step_is_unchanged(monkeypatch):
    x, xt, y = _batch()
    ce, bce = losses.CrossEntropyLoss(ignore_index=19), losses.BCEWithLogitsLoss()
    spy = _Spy(monkeypatch)
    res = []
    for fuse in (False, True):
        monkeypatch.setattr(F, "FUSE_REDUCE_ADAM", fuse)
        with rtsds_amd.precision(torch.bfloat16):
            torch.manual_seed(6)
            net = BiSeNet(19, "resnet18").to(DEV).train()
            disc = TinyDomainDiscriminator(19).to(DEV).train()
            opt = optim.Adam(net.parameters(), lr=1e-3)
            dopt = optim.Adam(disc.parameters(), lr=1e-3, weight_decay=1e-4)
            logs = [float(v) for v in rtrain.da_step(net, disc, opt, dopt, ce, bce, x, y, xt, 0.1, 2)]
            torch.cuda.synchronize()
            st = _snapshot(net, [opt, dopt])
            st.update({"D." + k: v.detach().clone() for k, v in disc.state_dict().items()})
            res.append((logs, st))
    assert spy.taken == 0 and spy.refused == 0  # several backward passes accumulate: never handed over
    assert res[0][0] == res[1][0]
    _same(res[0][1], res[1][1])
