"""Prediction path, CPU side: the numpy restatement tests/paint_ref.py on hand-computed values,
the host refusals of rtsds_upsample_paint (they return before any HIP call, so no device is
needed), the tables and the argument parser of rtsds_amd.predict, and the refusal of CPU models
and tensors."""
import numpy as np
import pytest
import torch

from rtsds_amd import _lib, predict
from rtsds_amd import functional as F
from rtsds_amd.datasets.gta5 import TRAIN_ID_COLORS
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet
from tests import paint_ref as R


# ----------------------------------------------------------------------------- restatement
def test_paint_ref_ends_of_the_range():
    rng = np.random.default_rng(0)
    classes = rng.integers(0, 19, (5, 7))
    frame = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    pal = np.array(TRAIN_ID_COLORS, np.uint8)
    assert np.array_equal(R.paint_ref(classes, pal, 256, frame), pal[classes])
    assert np.array_equal(R.paint_ref(classes, pal, 256), pal[classes])  # no frame needed
    assert np.array_equal(R.paint_ref(classes, pal, 0, frame), frame)
    assert R.paint_ref(classes, pal, 77, frame).dtype == np.uint8


def test_paint_ref_rounding_hand_cases():
    one = lambda p, f, a: int(R.paint_ref([0], [[p, p, p]], a, np.array([[f, f, f]], np.uint8))[0, 0])  # noqa: E731
    assert one(255, 0, 1) == 1        # (255 + 128) >> 8 = 383 >> 8
    assert one(0, 255, 255) == 1      # the mirror image
    assert one(127, 0, 1) == 0        # (127 + 128) >> 8 = 255 >> 8: just below one half
    assert one(128, 0, 1) == 1        # (128 + 128) >> 8 = 1: exactly one half rounds up
    assert one(1, 0, 128) == 1        # (128 + 128) >> 8: 0.5 again, from the other factor
    assert one(255, 255, 100) == 255  # a constant stays: (255 * 256 + 128) >> 8
    assert one(0, 0, 100) == 0
    assert one(200, 100, 128) == 150  # (25600 + 12800 + 128) >> 8 = 38528 >> 8
    assert one(201, 100, 128) == 151  # 150.5 rounds up


def test_ids_ref():
    classes = np.array([[0, 18], [3, 3]])
    assert R.ids_ref(classes).tolist() == [[0, 18], [3, 3]] and R.ids_ref(classes).dtype == np.uint8
    assert R.ids_ref(classes, predict.CITYSCAPES_LABEL_IDS).tolist() == [[7, 33], [12, 12]]


# ----------------------------------------------------------------------------- C entry
def test_binding_and_abi():
    assert _lib.ABI_VERSION >= 20
    res, args = _lib.SIGNATURES["rtsds_upsample_paint"]
    assert res is _lib.c_int and len(args) == 17
    assert _lib.load().rtsds_upsample_paint


def test_entry_refuses_bad_arguments_on_the_host():
    """Every guard returns before a launch: callable without a device, with made-up addresses."""
    lib = _lib.load()
    X, FR, PAL, IDS, RGB = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000

    def up(x=X, frame=FR, pal=PAL, ids=IDS, rgb=RGB, n=1, hi=2, wi=2, c=19, ho=4, wo=4, a=128):
        return lib.rtsds_upsample_paint(x, frame, pal, None, ids, rgb, n, hi, wi, c, ho, wo, 0.5, 0.5, a, 0, None)
    assert up(c=1) == 1 and up(c=33) == 1                    # c outside [2, 32]
    assert up(a=-1) == 1 and up(a=257) == 1                  # alpha_q8 outside [0, 256]
    for zero in ("n", "hi", "wi", "ho", "wo"):
        assert up(**{zero: 0}) == 1, zero                    # a zero size
    assert up(n=-1) == 1
    assert up(x=None) == 2                                   # no input
    assert up(ids=None, rgb=None) == 2                       # no output
    assert up(pal=None) == 2                                 # rgb without a palette
    assert up(frame=None, a=255) == 2 and up(frame=None, a=0) == 2  # a blend without the frame
    assert up(n=1 << 16, ho=1 << 16, wo=256) == 2            # 2^32 blocks: beyond INT_MAX
    assert up(c=1, x=None) == 1                              # the shape is judged first


# ----------------------------------------------------------------------------- predict
def test_cityscapes_label_ids():
    ids = predict.CITYSCAPES_LABEL_IDS
    assert ids == (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33)
    assert len(ids) == 19 and len(set(ids)) == 19 and list(ids) == sorted(ids)


def test_default_palette_is_the_one_gta5_decode_inverts():
    pal = predict.default_palette()
    assert pal.dtype == torch.uint8 and pal.tolist() == [list(c) for c in TRAIN_ID_COLORS]
    assert len({tuple(c) for c in pal.tolist()}) == 19  # invertible


def test_argument_parser():
    a = predict.argument_parser(["--weights", "w.pth", "--input", "in", "--output", "out"])
    assert (a.model, a.overlay, a.label_ids, a.batch_size) == ("bisenet", 1.0, False, 1)
    assert a.config.endswith("config.yaml")
    a = predict.argument_parser(["--config", "c.yaml", "--model", "deeplab", "--weights", "w.pth", "--input", "in",
                                 "--output", "out", "--overlay", "0.4", "--label_ids", "--batch_size", "8"])
    assert (a.config, a.model, a.weights, a.input, a.output) == ("c.yaml", "deeplab", "w.pth", "in", "out")
    assert (a.overlay, a.label_ids, a.batch_size) == (0.4, True, 8)
    with pytest.raises(SystemExit):
        predict.argument_parser(["--input", "in", "--output", "out"])  # the weights are not optional
    with pytest.raises(SystemExit):
        predict.argument_parser(["--weights", "w", "--input", "in", "--output", "out", "--model", "unet"])


def test_input_paths(tmp_path):
    for name in ("b.png", "a.JPG", "c.jpeg", "notes.txt"):
        (tmp_path / name).write_bytes(b"")
    got = predict.input_paths(str(tmp_path))
    assert [p.rsplit("/", 1)[1] for p in got] == ["a.JPG", "b.png", "c.jpeg"]
    assert predict.input_paths(str(tmp_path / "b.png")) == [str(tmp_path / "b.png")]
    with pytest.raises(RuntimeError, match="does not exist"):
        predict.input_paths(str(tmp_path / "missing.png"))


def test_cpu_models_and_tensors_are_refused():
    x = torch.zeros(1, 19, 4, 8)
    geo = F.upsample_geometry(x, size=(32, 64))
    with pytest.raises(RuntimeError, match="^rtsds_amd: upsample_paint"):
        F.upsample_paint(x, geo)
    with pytest.raises(RuntimeError, match="^rtsds_amd: upsample_paint"):
        F.upsample_paint(x, geo, palette=predict.default_palette(), alpha=0.5, frame=torch.zeros(1, 32, 64, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="^rtsds_amd: Predictor needs a model on a HIP device"):
        predict.Predictor(BiSeNet(19, "resnet18"), (64, 128))
    with pytest.raises(RuntimeError, match="forward_lowres"):
        predict.Predictor(torch.nn.Conv2d(3, 19, 1), (64, 128))
