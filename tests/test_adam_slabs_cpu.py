"""The host-side planning of the fused reduce + Adam step (optim.slab_plan, optim.zero_plan) and the
dirty-range bookkeeping of zero_grad, on a hand-made arena layout.  No device: the arena is a stub
around a CPU gradient buffer and the zero-fill entry is replaced by a recorder that fills on the host."""
import torch

from rtsds_amd import optim

# five parameters in 64-float segments: a conv weight (128), its BatchNorm pair (2 x 16), a 1-element
# parameter, a second conv weight (64, filling its segment)
OFFSETS = [0, 128, 192, 256, 320]
NUMEL = [128, 16, 16, 1, 64]
TOTAL = 384


def test_zero_plan_merges_neighbours_and_takes_whole_segments():
    assert optim.zero_plan(OFFSETS, TOTAL, [False] * 5) == []
    assert optim.zero_plan(OFFSETS, TOTAL, [True] * 5) == [(0, TOTAL)]
    assert optim.zero_plan(OFFSETS, TOTAL, [False, True, True, False, False]) == [(128, 256)]
    assert optim.zero_plan(OFFSETS, TOTAL, [True, False, True, True, False]) == [(0, 128), (192, 320)]
    assert optim.zero_plan(OFFSETS, TOTAL, [False, False, False, False, True]) == [(320, 384)]


def test_slab_plan_sorts_and_lists_the_holes():
    # handed over in backward order: the later weight first
    order, holes = optim.slab_plan(0, 384, [(320, 64), (0, 128)])
    assert order == [1, 0] and holes == [(0, 128), (320, 384)]
    # holes adjacent to each other, at the very start and the very end of the run
    order, holes = optim.slab_plan(128, 384, [(128, 64), (192, 64), (320, 64)])
    assert order == [0, 1, 2] and holes == [(128, 192), (192, 256), (320, 384)]
    assert optim.slab_plan(0, 384, []) == ([], [])


def test_slab_plan_refuses_what_one_launch_cannot_cover_exactly_once():
    assert optim.slab_plan(0, 384, [(0, 128), (0, 128)]) is None      # the same gradient reduced twice
    assert optim.slab_plan(0, 384, [(0, 128), (64, 64)]) is None      # overlapping
    assert optim.slab_plan(128, 384, [(0, 128)]) is None              # before the run
    assert optim.slab_plan(0, 320, [(320, 64)]) is None               # behind the run
    assert optim.slab_plan(0, 384, [(320, 68)]) is None               # past its end
    assert optim.slab_plan(0, 384, [(2, 64)]) is None                 # not on a 16-B vector
    assert optim.slab_plan(0, 384, [(0, 6)]) is None                  # not whole vectors
    assert optim.slab_plan(0, 384, [(0, 0)]) is None


class _P:
    grad = None

    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


def _stub(monkeypatch):
    a = optim._Arena.__new__(optim._Arena)
    n = len(OFFSETS)
    a.params, a.offsets, a.total = [_P(k) for k in NUMEL], list(OFFSETS), TOTAL
    a.gflat = torch.zeros(TOTAL)
    a.touched, a.dirty, a.lazy, a._was_dirty = ([False] * n for _ in range(4))
    a.gen, a.reduced, a._gver = [0] * n, None, a.gflat._version
    monkeypatch.setattr(optim._Arena, "grad_ptr_ok", lambda self, i: True)
    opt = optim.Adam.__new__(optim.Adam)
    opt._arenas, opt._pending = [a], ["stale"]
    fills = []

    class Lib:
        @staticmethod
        def rtsds_zero_ranges(ptr, count, lo, hi, st):
            rng = [(lo[k], hi[k]) for k in range(count)]
            fills.append(rng)
            for x, y in rng:
                a.gflat[x:y] = 0

    monkeypatch.setattr(optim, "lib", Lib)
    monkeypatch.setattr(optim, "stream", lambda: 0)
    return opt, a, fills


def _write(a, i):
    a.sink(i)
    a.gflat[a.offsets[i]:a.offsets[i] + a.params[i].numel()] = 1.0


def test_zero_grad_fills_only_what_was_written(monkeypatch):
    opt, a, fills = _stub(monkeypatch)
    opt.zero_grad()
    assert fills == [] and opt._pending == []                      # a fresh arena is clean
    # a fused step: the weights' sinks handed out but deferred, the BatchNorm pair written
    for i in (0, 4):
        a.sink(i)
        a.sink_unwritten(i)
    _write(a, 1)
    _write(a, 2)
    assert a.dirty == [False, True, True, False, False] and a.touched == [True, True, True, False, True]
    opt.zero_grad()
    assert fills == [[(128, 256)]] and not a.gflat.any()
    assert not any(a.dirty) and not any(a.touched) and not any(a.lazy)
    # a fallback step: weight 0's reduction was materialised into the arena (functional.reduce_wgrads_now)
    a.sink(0)
    a.sink_unwritten(0)
    a.dirty[0] = True
    a.gflat[0:128] = 2.0
    opt.zero_grad()
    assert fills[-1] == [(0, 128)] and not a.gflat.any()
    # written first, deferred afterwards: the range holds the earlier contribution and stays dirty
    _write(a, 4)
    a.sink(4)
    a.sink_unwritten(4)
    assert a.dirty[4]
    # a caller that sets touched by hand after writing .grad in place is still zeroed
    a.touched[3] = True
    a.gflat[256] = 3.0
    opt.zero_grad()
    assert fills[-1] == [(256, 384)] and not a.gflat.any()
    # everything written: one fill of the whole arena, as before
    for i in range(5):
        _write(a, i)
    n = len(fills)
    opt.zero_grad()
    assert len(fills) == n and not a.gflat.any()


def test_grad_hook_dirties_only_after_a_real_accumulate(monkeypatch):
    opt, a, fills = _stub(monkeypatch)
    a._hook(1)(None)                       # the Function returned None: nothing was added
    assert a.touched[1] and not a.dirty[1]
    a.gflat[128:144] += 1.0                # AccumulateGrad's in-place add bumps the buffer's version
    a._hook(1)(None)
    assert a.dirty[1]
    opt.zero_grad()
    assert fills == [[(128, 192)]] and not a.gflat.any()
    a._hook(2)(None)                       # zero_grad's own fill is not taken for a gradient
    assert not a.dirty[2]
