"""Paired random scale-crop without a GPU: RandomResizedCrop's draws against an independent
restatement (tests/cropaug_ref.py), the config loader, the order of a sample's draws, the
argument validation of rtsds_crop_resize_aa / rtsds_crop_resize_nearest (which comes before any
launch), the label pipeline's refusals and the hand-over of the geometry in DeviceLoader."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch
import yaml

from rtsds_amd import _lib
from rtsds_amd import transforms as T

from tests import cropaug_ref as R


# ------------------------------------------------------------------ RandomResizedCrop.params
@pytest.mark.parametrize("hw", [(37, 53), (1052, 1914)])
@pytest.mark.parametrize("kwargs", [{}, {"scale": (0.25, 1.0), "ratio": (1.5, 2.1)}])
def test_params_match_the_restatement_and_leave_the_generator_alike(hw, kwargs):
    rrc = T.RandomResizedCrop(**kwargs)
    for seed in range(200):
        torch.manual_seed(seed)
        got = rrc.params(*hw)
        after = torch.rand(1)
        torch.manual_seed(seed)
        want = R.get_params(*hw, rrc.scale, rrc.ratio)
        assert got == want, (seed, got, want)
        assert torch.equal(after, torch.rand(1)), seed
        assert R.inside(got, *hw), (seed, got)
        assert all(isinstance(v, int) for v in got)


def test_defaults_are_torchvisions():
    rrc = T.RandomResizedCrop()
    assert rrc.scale == (0.08, 1.0) and rrc.ratio == (3.0 / 4.0, 4.0 / 3.0)


def _after_uniforms(seed, n):
    """The generator's next value after n uniform_ draws of one element."""
    torch.manual_seed(seed)
    for _ in range(n):
        torch.empty(1).uniform_(0.0, 1.0)
    return torch.rand(1)


@pytest.mark.parametrize("hw,want", [((40, 50), (0, 0, 40, 50)),      # 1.25 lies in (3/4, 4/3): the whole image
                                     ((37, 53), (0, 2, 37, 49)),      # 1.43 > 4/3: full height, width round(37 * 4/3)
                                     ((53, 37), (2, 0, 49, 37))])     # 0.70 < 3/4: full width, height round(37 / (3/4))
def test_fallback_after_twenty_uniforms_and_no_randint(hw, want):
    """scale = (4, 4): four times the image's area never fits."""
    rrc = T.RandomResizedCrop(scale=(4, 4))
    torch.manual_seed(5)
    assert rrc.params(*hw) == want
    assert torch.equal(torch.rand(1), _after_uniforms(5, 20))


def test_fallback_clamps_the_ratio_on_a_two_to_one_image():
    # the whole area at 3 : 1 is 122 wide: never fits in 100
    assert T.RandomResizedCrop(scale=(1, 1), ratio=(3, 3)).params(50, 100) == (8, 0, 33, 100)
    # ... and at 1 : 2 it is 100 high: never fits in 50
    assert T.RandomResizedCrop(scale=(1, 1), ratio=(0.5, 0.5)).params(50, 100) == (0, 37, 50, 25)


@pytest.mark.parametrize("kwargs", [
    {"scale": (1.0, 0.5)}, {"ratio": (2.0, 1.0)},                      # descending
    {"scale": (0.0, 1.0)}, {"scale": (-0.1, 1.0)}, {"ratio": (0, 1)},  # not positive
    {"scale": 0.5}, {"ratio": (1.0,)}, {"scale": (0.1, 0.5, 1.0)}, {"ratio": ("a", "b")}, {"scale": None},
    {"scale": (0.5, float("inf"))}, {"ratio": (float("nan"), 1.0)},
])
def test_bad_ranges_raise_value_error(kwargs):
    with pytest.raises(ValueError):
        T.RandomResizedCrop(**kwargs)


# ------------------------------------------------------------------ augmentation_loader
def _config(aug):
    return SimpleNamespace(augmentation=aug)


def test_augmentation_loader_keeps_key_order_and_parses_strings():
    ra = T.augmentation_loader(_config({
        "p": 0.5,
        "RandomResizedCrop": {"scale": "0.25, 1.0", "ratio": "1.5, 2.1"},
        "GaussianBlur": {"kernel_size": "5, 9", "sigma": "0.1, 5"},
        "RandomHorizontalFlip": {"p": 0.5, "labels": True},
    }), 0.5)
    crop, blur, flip = ra.transforms
    assert isinstance(crop, T.RandomResizedCrop) and crop.scale == (0.25, 1.0) and crop.ratio == (1.5, 2.1)
    assert isinstance(blur, T.GaussianBlur)
    assert isinstance(flip, T.RandomHorizontalFlip) and flip.p == 0.5 and flip.labels is True


def test_augmentation_loader_defaults():
    ra = T.augmentation_loader(_config({"p": 0.5, "RandomHorizontalFlip": {"p": 0.25}, "RandomResizedCrop": {}}), 0.5)
    flip, crop = ra.transforms
    assert flip.labels is False and flip.p == 0.25
    assert crop.scale == (0.08, 1.0) and crop.ratio == (3.0 / 4.0, 4.0 / 3.0)
    assert T.RandomHorizontalFlip().labels is False


def test_shipped_config_example_uncommented():
    """config.yaml carries the crop and the paired flip as a commented example; uncommented
    (in place of the image-only flip) it loads."""
    text = open(os.path.join(os.path.dirname(T.__file__), "config.yaml")).read()
    lines = text.split("\n")
    for example in ('  # RandomHorizontalFlip: {p: 0.5, labels: true}',
                    '  # RandomResizedCrop: {scale: "0.25, 1.0", ratio: "1.5, 2.1"}'):
        lines[lines.index(example)] = example.replace("# ", "", 1)
    lines.remove("  RandomHorizontalFlip: {p: 0.5}")
    aug = yaml.safe_load("\n".join(lines))["augmentation"]
    ra = T.augmentation_loader(_config(aug), 0.5)
    assert [type(t) for t in ra.transforms] == [T.GaussianBlur, T.RandomHorizontalFlip, T.RandomResizedCrop]
    assert ra.transforms[1].labels is True and ra.transforms[2].ratio == (1.5, 2.1)
    # as shipped: no crop, the reference's image-only flip
    shipped = T.augmentation_loader(_config(yaml.safe_load(text)["augmentation"]), 0.5)
    assert [type(t) for t in shipped.transforms] == [T.GaussianBlur, T.RandomHorizontalFlip]
    assert shipped.transforms[1].labels is False


# ------------------------------------------------------------------ draw order
def test_sample_draws_coin_sigma_window_flip():
    blur = T.GaussianBlur((5, 9), (0.1, 5.0))
    crop = T.RandomResizedCrop(scale=(0.25, 1.0), ratio=(1.5, 2.1))
    ra = T.RandomApply([blur, crop, T.RandomHorizontalFlip(0.5, labels=True)], p=1.0)
    for seed in range(20):
        torch.manual_seed(seed)
        ops, flip, window, flip_label = T._sample_draws(ra, 64, 96)
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        torch.rand(1)                                                # RandomApply's coin
        sigma = float(torch.empty(1).uniform_(0.1, 5.0))            # GaussianBlur.get_params
        want_window = R.get_params(64, 96, (0.25, 1.0), (1.5, 2.1))  # RandomResizedCrop.get_params
        want_flip = bool(torch.rand(1) < 0.5)                        # the flip's coin
        assert torch.equal(state, torch.get_rng_state())
        assert [t for t, _ in ops] == [blur] and ops[0][1] == sigma
        assert window == want_window and flip == want_flip and flip_label == want_flip


def test_failed_coin_draws_nothing_else_and_unpaired_flip_is_not_for_the_label():
    ra = T.RandomApply([T.RandomResizedCrop(), T.RandomHorizontalFlip(1.0)], p=0.0)
    torch.manual_seed(3)
    assert T._sample_draws(ra, 64, 96) == ([], False, None, False)
    state = torch.get_rng_state()
    torch.manual_seed(3)
    torch.rand(1)
    assert torch.equal(state, torch.get_rng_state())
    ra.p = 1.0
    _, flip, window, flip_label = T._sample_draws(ra, 64, 96)
    assert flip is True and flip_label is False and window is not None


def test_decisions_keeps_its_two_tuple_and_its_draws():
    """A list without the crop: coin, sigma, flip coin as before; with the crop _decisions has no
    source size to draw for and says so."""
    ra = T.RandomApply([T.GaussianBlur((5, 9), (0.1, 5.0)), T.RandomHorizontalFlip(0.5, labels=True)], p=1.0)
    torch.manual_seed(2)
    ops, flip = T._decisions(ra)
    state = torch.get_rng_state()
    torch.manual_seed(2)
    torch.rand(1)
    sigma = float(torch.empty(1).uniform_(0.1, 5.0))
    want_flip = bool(torch.rand(1) < 0.5)
    assert torch.equal(state, torch.get_rng_state())
    assert len(ops) == 1 and ops[0][1] == sigma and flip == want_flip
    assert T._decisions(None) == ([], False)
    with pytest.raises(RuntimeError, match="source size"):
        T._decisions(T.RandomApply([T.RandomResizedCrop()], p=1.0))


# ------------------------------------------------------------------ C entry points
OK, SHAPE, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4


def _aa(**over):
    """rtsds_crop_resize_aa with valid arguments except those overridden; host memory stands in
    for the device pointers (validation returns before anything is launched)."""
    lib = _lib.load()
    a = dict(src_u8=1, c=3, h=64, w=96, y0=8, x0=16, hc=40, wc=60, kind=0, ho=32, wo=48, flip=0, mean=None, stdv=None,
             short=0)
    a.update(over)
    need = int(lib.rtsds_resize_aa_workspace(a["c"], a["hc"], a["wc"], a["ho"], a["wo"]))
    buf = ctypes.create_string_buffer(max(need, 64))
    p = ctypes.addressof(buf)
    rc = lib.rtsds_crop_resize_aa(a.get("src", p), a["src_u8"], a["c"], a["h"], a["w"], a["y0"], a["x0"], a["hc"],
                                  a["wc"], a.get("dst", p), a["kind"], a["ho"], a["wo"], a["flip"], a["mean"],
                                  a["stdv"], 0, -1, a.get("ws", p), need - a["short"], None)
    del buf
    return rc


def _nearest(**over):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    a = dict(src=p, src_i64=0, h=64, w=96, y0=8, x0=16, hc=40, wc=60, dst=p, ho=32, wo=48, flip=0)
    a.update(over)
    rc = _lib.load().rtsds_crop_resize_nearest(a["src"], a["src_i64"], a["h"], a["w"], a["y0"], a["x0"], a["hc"],
                                               a["wc"], a["dst"], a["ho"], a["wo"], a["flip"], 0, -1, None)
    del buf
    return rc


BAD_WINDOWS = [{"y0": -1}, {"x0": -1}, {"y0": 25}, {"x0": 37},            # past each of the four borders by one
               {"hc": 65, "y0": 0}, {"wc": 97, "x0": 0},                  # larger than the image
               {"hc": 0}, {"wc": 0}, {"hc": -3}, {"h": 0}, {"w": -1},
               {"y0": 2 ** 31 - 1}, {"x0": 2 ** 31 - 1},                  # no wrap-around in y0 + hc
               {"ho": 0}, {"wo": -2}, {"src": None}, {"dst": None}]


@pytest.mark.parametrize("over", BAD_WINDOWS)
def test_both_entries_refuse_bad_windows(over):
    assert _aa(**over) == SHAPE
    assert _nearest(**over) == SHAPE


@pytest.mark.parametrize("over", [{"c": 0}, {"kind": 3}, {"kind": -1}, {"mean": 1}, {"stdv": 1}])
def test_aa_entry_refuses_bad_arguments(over):
    """mean / std given singly (any non-null pointer: nothing is dereferenced)."""
    if "mean" in over or "stdv" in over:
        buf = ctypes.create_string_buffer(16)
        over = {k: ctypes.addressof(buf) for k in over}
    assert _aa(**over) == SHAPE


def test_aa_entry_tap_limit_and_workspace():
    wide = dict(h=8, w=2048, y0=0, x0=0, hc=8, wc=2048, ho=8, wo=32)  # 64x down: 129 taps
    assert _aa(**wide) == UNSUPPORTED
    assert _aa(short=1) == WORKSPACE
    assert _aa(ws=None) == WORKSPACE
    # the window sizes the workspace, not the image
    lib = _lib.load()
    assert lib.rtsds_resize_aa_workspace(3, 40, 60, 32, 48) < lib.rtsds_resize_aa_workspace(3, 64, 96, 32, 48)
    # bad shapes are reported before the workspace
    assert _aa(hc=0, short=1) == SHAPE and _aa(**dict(wide, short=1)) == UNSUPPORTED


# ------------------------------------------------------------------ LabelPipeline / DeviceLoader
def test_label_pipeline_refuses_mismatched_geometry():
    lp = T.LabelPipeline((8, 8))
    labs = [torch.zeros(16, 24, dtype=torch.uint8), torch.zeros(16, 24, dtype=torch.int64)]
    with pytest.raises(RuntimeError, match="geometry of 1 samples for 2 labels"):
        lp(labs, [None])
    with pytest.raises(RuntimeError, match="geometry of 3 samples"):
        lp(labs, [None, None, None])
    window = T.Geometry(1, 2, 8, 8, False, source=(32, 24))
    for lab in labs:
        with pytest.raises(RuntimeError, match="label of 16 x 24 for a window drawn in an image of 32 x 24"):
            lp([lab], [window])
    with pytest.raises(RuntimeError, match="uint8 or int64"):
        lp([torch.zeros(16, 24)], [T.Geometry(1, 2, 8, 8, False, source=(16, 24))])
    with pytest.raises(RuntimeError, match="single-channel"):
        lp([torch.zeros(16, 24, 3, dtype=torch.uint8)], [T.Geometry(1, 2, 8, 8, False, source=(16, 24))])


def test_geometry_is_the_five_tuple_with_the_source_size():
    g = T.Geometry(1, 2, 8, 9, 1, source=(16, 24))
    assert g == (1, 2, 8, 9, True) and g.source == (16, 24) and len(g) == 5
    assert T.ImagePipeline((8, 8)).last_geometry is None


class _ImagePipe:
    def __init__(self, geometry):
        self.seen, self.last_geometry, self._geometry = [], None, geometry

    def __call__(self, images):
        self.seen.append(images)
        self.last_geometry = self._geometry[len(self.seen) - 1]
        return len(images)


class _LabelPipe:
    def __init__(self):
        self.seen = []

    def __call__(self, labels, geometry="absent"):
        self.seen.append((labels, geometry))
        return len(labels)


def test_device_loader_hands_the_geometry_across():
    batches = [([torch.zeros(4, 6, 3, dtype=torch.uint8)] * 2, [torch.zeros(4, 6, dtype=torch.uint8)] * 2),
               ([torch.zeros(5, 7, 3, dtype=torch.uint8)], [torch.zeros(5, 7, dtype=torch.uint8)])]
    geo = [[None, T.Geometry(0, 1, 2, 3, True, source=(4, 6))], [None]]
    ip, lp = _ImagePipe(geo), _LabelPipe()
    assert list(T.DeviceLoader(batches, ip, lp, device="cpu")) == [(2, 2), (1, 1)]
    assert [g for _, g in lp.seen] == geo and lp.seen[0][1] is geo[0]
    assert [len(l) for l, _ in lp.seen] == [2, 1]
    # an image pipe without the record: the label pipe is called as before
    lp = _LabelPipe()
    assert list(T.DeviceLoader(batches, lambda t: len(t), lp, device="cpu")) == [(2, 2), (1, 1)]
    assert [g for _, g in lp.seen] == ["absent", "absent"]
