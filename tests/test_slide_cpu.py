"""Sliding-window prediction, CPU side: the window grid (validation.sliding_windows and its numpy
restatement tests/slide_ref.py) on hand-computed values, the host refusals of rtsds_slide_paint
(they return before any HIP call, so no device is needed), the new keyword arguments and parser
options, and the refusal of CPU models and tensors."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from rtsds_amd import _lib, predict, validation
from rtsds_amd import functional as F
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet
from tests import slide_ref as S


# ----------------------------------------------------------------------------- the grid
def _axis(S_, w, s):
    """One axis of sliding_windows (the other axis a single window)."""
    got = validation.sliding_windows((S_, 5), (w, 5), (s, 1))
    assert [x0 for _, x0 in got] == [0] * len(got)
    assert [y0 for y0, _ in got] == S.axis_origins(S_, w, s)
    return [y0 for y0, _ in got]


def test_grid_by_hand():
    assert _axis(40, 32, 8) == [0, 8]
    assert _axis(80, 48, 16) == [0, 16, 32]
    assert _axis(300, 96, 68) == [0, 68, 136, 204]
    assert _axis(64, 64, 32) == [0]            # S == w
    assert _axis(50, 32, 100) == [0, 18]       # a stride larger than S - w
    # row-major, both axes, and the default stride of half the window
    assert validation.sliding_windows((40, 80), (32, 48), (8, 16)) == [(0, 0), (0, 16), (0, 32), (8, 0), (8, 16), (8, 32)]
    assert validation.sliding_windows((40, 80), (32, 48), (8, 16)) == S.windows_ref((40, 80), (32, 48), (8, 16))
    assert validation.sliding_windows((64, 96), (32, 48)) == validation.sliding_windows((64, 96), (32, 48), (16, 24))
    assert validation.sliding_windows((64, 96), (32, 48), None) == [(y, x) for y in (0, 16, 32) for x in (0, 24, 48)]


def test_grid_sweep_covers_every_pixel_once_per_origin():
    for S_, w, s in itertools.product(range(1, 24), range(1, 9), range(1, 11)):
        if S_ < w:
            continue
        o = _axis(S_, w, s)
        assert len(set(o)) == len(o) and o == sorted(o) and o[0] == 0 and o[-1] == S_ - w, (S_, w, s)
        covered = np.zeros(S_, bool)
        for a in o:
            covered[a:a + w] = True
        assert all(b - a <= s for a, b in zip(o, o[1:])), (S_, w, s)
        # windows never more than a stride apart: no gap exactly when the stride does not exceed the
        # window (a larger stride skips pixels by the rule itself; rtsds_slide_paint leaves them zero)
        assert covered.all() == (s <= w or len(o) == 1 or all(b - a <= w for a, b in zip(o, o[1:]))), (S_, w, s)
        if s <= w:
            assert covered.all(), (S_, w, s)


def test_grid_refusals():
    with pytest.raises(RuntimeError, match="^rtsds_amd: sliding_windows"):
        validation.sliding_windows((31, 64), (32, 48), (8, 8))   # S < w
    with pytest.raises(RuntimeError, match="^rtsds_amd: sliding_windows"):
        validation.sliding_windows((64, 47), (32, 48), (8, 8))
    with pytest.raises(RuntimeError, match="^rtsds_amd: sliding_windows"):
        validation.sliding_windows((64, 64), (32, 48), (0, 8))   # a stride < 1
    with pytest.raises(RuntimeError, match="^rtsds_amd: sliding_windows"):
        validation.sliding_windows((64, 64), (32, 48), (8, -1))


def test_slide_table_and_chunks():
    t = validation.slide_table((40, 80), (32, 48), (8, 16), flip=True)
    assert len(t) == 12 and t[:4] == [(0, 0, 0), (0, 0, 1), (0, 16, 0), (0, 16, 1)]
    assert validation.slide_table((40, 80), (32, 48), (8, 16)) == [(y, x, 0) for y, x in S.windows_ref((40, 80), (32, 48), (8, 16))]
    assert [len(c) for c in validation.slide_chunks(t, 2, 16)] == [8, 4]
    assert [len(c) for c in validation.slide_chunks(t, 2, 1)] == [1] * 12     # max(1, 1 // 2)
    assert [len(c) for c in validation.slide_chunks(t, 1, 1000)] == [12]
    assert [len(c) for c in validation.slide_chunks(t * 11, 1, 1000)] == [64, 64, 4]  # the entry's own limit


# ----------------------------------------------------------------------------- restatement
def test_covering_sum_and_argmax_by_hand():
    p0 = np.full((1, 2, 2, 2), 0.25, np.float32)
    p1 = np.array([0.5, 0.125], np.float32) * np.ones((1, 2, 2, 2), np.float32)
    s = S.covering_sum([p0, p1], [(0, 0, 0), (1, 1, 0)], (3, 4))
    assert s.dtype == np.float32 and s.shape == (1, 3, 4, 2)
    assert s[0, 0, 0].tolist() == [0.25, 0.25] and s[0, 2, 2].tolist() == [0.5, 0.125]
    assert s[0, 1, 1].tolist() == [0.75, 0.375] and s[0, 0, 3].tolist() == [0.0, 0.0]
    assert S.argmax_first(s)[0].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    old = np.full((1, 3, 4, 2), 2.0, np.float32)
    s = S.covering_sum([p0], [(0, 0)], (3, 4), acc=old)
    assert s[0, 0, 0].tolist() == [2.25, 2.25] and s[0, 2, 3].tolist() == [2.0, 2.0] and old.max() == 2.0
    # float32 adds, in window order: (1 + 2^-24) + 2^-24 stays 1, 2^-24 + 2^-24 + 1 does not
    one, eps = np.ones((1, 1, 1, 2), np.float32), np.full((1, 1, 1, 2), 2.0 ** -24, np.float32)
    assert S.covering_sum([one, eps, eps], [(0, 0)] * 3, (1, 1)).max() == 1.0
    assert S.covering_sum([eps, eps, one], [(0, 0)] * 3, (1, 1)).max() > 1.0
    assert S.argmax_first(np.array([[1.0, 3.0, 3.0], [2.0, 2.0, 1.0], [0.0, 0.0, 0.0]])).tolist() == [1, 0, 0]


# ----------------------------------------------------------------------------- C entry
def test_binding_and_abi():
    assert _lib.ABI_VERSION >= 21
    res, args = _lib.SIGNATURES["rtsds_slide_paint"]
    assert res is _lib.c_int and len(args) == 23
    assert _lib.load().rtsds_slide_paint


def test_entry_refuses_bad_arguments_on_the_host():
    """Every guard returns before a launch: callable without a device, with made-up addresses."""
    lib = _lib.load()
    X, FR, PAL, ACC, IDS, RGB = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000

    def sp(x=X, win=((0, 0, 0), (8, 32, 1)), nwin=None, frame=FR, pal=PAL, acc=ACC, ids=IDS, rgb=RGB, nf=1, hi=4, wi=6, c=19,
           hw=32, ww=48, H=40, W=80, accumulate=0, a=128, dtype=0):
        flat = [v for w in win for v in w]
        arr = (ctypes.c_int * max(1, len(flat)))(*flat)
        return lib.rtsds_slide_paint(x, arr, len(win) if nwin is None else nwin, frame, pal, None, acc, ids, rgb, nf, hi, wi, c,
                                     hw, ww, H, W, 0.125, 0.125, accumulate, a, dtype, None)
    for y0, x0 in ((9, 0), (0, 33), (-1, 0), (0, -1)):
        assert sp(win=((0, 0, 0), (y0, x0, 0))) == 1, (y0, x0)  # a window outside the canvas
    assert sp(win=(), nwin=0) == 1                            # no window
    assert sp(win=((0, 0, 0),) * 65) == 2                     # more than 64: the caller chunks
    assert sp(win=((0, 0, 0),) * 64, x=None) == 2             # 64 pass the count (and fail on x)
    assert sp(c=1) == 1 and sp(c=33) == 1                     # c outside [2, 32]
    assert sp(a=-1) == 1 and sp(a=257) == 1                   # alpha_q8 outside [0, 256]
    for zero in ("nf", "hi", "wi", "hw", "ww", "H", "W"):
        assert sp(**{zero: 0}) == 1, zero                     # a zero size
    assert sp(hw=41) == 1 and sp(ww=81) == 1                  # a window larger than the canvas
    assert sp(acc=None, ids=None, rgb=None) == 2              # no output
    assert sp(acc=None, accumulate=1) == 2                    # accumulate without acc
    assert sp(x=None) == 2 and sp(pal=None) == 2              # no input; rgb without a palette
    assert sp(frame=None, a=255) == 2 and sp(frame=None, a=0) == 2  # a blend without the frame
    assert sp(dtype=7) == 2                                   # a bad dtype
    assert sp(nf=1 << 16, H=1 << 16, hw=32, W=256) == 2       # 2^32 blocks: beyond INT_MAX
    assert sp(c=1, x=None) == 1                               # the shape is judged first


# ----------------------------------------------------------------------------- Python surface
def test_argument_parser_options():
    base = ["--weights", "w.pth", "--input", "in", "--output", "out"]
    a = predict.argument_parser(base)
    assert (a.stride, a.flip, a.max_batch) == (None, False, 16)
    a = predict.argument_parser(base + ["--stride", "256,512", "--flip", "--max_batch", "4"])
    assert (a.stride, a.flip, a.max_batch) == ("256,512", True, 4)
    from rtsds_amd import transforms as T
    assert T.parse_size(a.stride) == [256, 512]


class _Loader(list):
    pass


def test_val_refuses_window_with_scales():
    net = torch.nn.Conv2d(3, 19, 1)
    with pytest.raises(RuntimeError, match="window together with scales"):
        validation.val(0, net, _Loader(), 19, window=(32, 64), scales=(1.0,))
    with pytest.raises(RuntimeError, match="window together with scales"):
        validation.val_GTA5(0, net, _Loader(), 19, ["a"] * 19, window=(32, 64), scales=(0.5, 1.0))


def test_cpu_models_and_tensors_are_refused():
    x = torch.zeros(2, 19, 4, 8)
    geo = F.upsample_geometry(x, size=(32, 64))
    with pytest.raises(RuntimeError, match="^rtsds_amd: slide_paint.*HIP"):
        F.slide_paint(x, geo, [(0, 0), (0, 32)], (32, 96), 1)
    with pytest.raises(RuntimeError, match="^rtsds_amd: slide_paint.*HIP"):
        F.slide_paint(x, geo, [(0, 0), (0, 32)], (32, 96), 1, acc=torch.zeros(1, 32, 96, 19))
    net = BiSeNet(19, "resnet18")
    with pytest.raises(RuntimeError, match="^rtsds_amd: predict_sliding.*HIP"):
        validation.predict_sliding(net, torch.zeros(1, 3, 64, 128), (64, 128))
    with pytest.raises(RuntimeError, match="forward_lowres"):
        validation.predict_sliding(torch.nn.Conv2d(3, 19, 1), torch.zeros(1, 3, 64, 128), (64, 128))
    with pytest.raises(RuntimeError, match="^rtsds_amd: Predictor needs a model on a HIP device"):
        predict.Predictor(net, (64, 128), stride=(32, 64), flip=True)


def test_predictor_stride_none_constructs_as_before():
    """The constructor's checks run in their old order with the new keywords left alone, and bad
    values of the new ones are refused only after a valid model: no device here, so the model check
    is what answers."""
    import inspect
    sig = inspect.signature(predict.Predictor.__init__)
    assert list(sig.parameters)[:7] == ["self", "model", "size", "palette", "label_ids", "alpha", "dtype"]
    assert (sig.parameters["stride"].default, sig.parameters["flip"].default, sig.parameters["max_batch"].default) == \
        (None, False, 16)
    with pytest.raises(RuntimeError, match="forward_lowres"):
        predict.Predictor(torch.nn.Conv2d(3, 19, 1), (64, 128), stride=None)
