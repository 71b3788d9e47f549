"""ColorJitter without a GPU: parameter handling, the config loader, the order of the draws
from torch's CPU generator, the argument validation of rtsds_color_jitter (which comes before
any HIP call), and the premises of the GPU parity tests (tests/colorjitter_ref.py)."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch
import yaml

from rtsds_amd import _lib
from rtsds_amd import transforms as T

from tests import colorjitter_ref as R


# ------------------------------------------------------------------ parameters
def test_numbers_become_ranges():
    cj = T.ColorJitter(brightness=0.2, contrast=0.5, saturation=1.5, hue=0.1)
    assert cj.brightness == pytest.approx((0.8, 1.2))
    assert cj.contrast == pytest.approx((0.5, 1.5))
    assert cj.saturation == pytest.approx((0.0, 2.5))  # floored at 0
    assert cj.hue == pytest.approx((-0.1, 0.1))
    assert cj.value_range == 255.0


def test_pairs_are_taken_as_given():
    cj = T.ColorJitter(brightness=(0.5, 2.0), contrast=[1.0, 1.5], saturation=(0, 0), hue=(-0.5, 0.25),
                       value_range=1.0)
    assert (cj.brightness, cj.contrast, cj.saturation, cj.hue) == ((0.5, 2.0), (1.0, 1.5), (0.0, 0.0), (-0.5, 0.25))
    assert cj.value_range == 1.0


def test_identity_ranges_switch_the_op_off():
    cj = T.ColorJitter()
    assert (cj.brightness, cj.contrast, cj.saturation, cj.hue) == (None, None, None, None)
    cj = T.ColorJitter(brightness=(1, 1), contrast=0.0, saturation=[1.0, 1.0], hue=(0, 0))
    assert (cj.brightness, cj.contrast, cj.saturation, cj.hue) == (None, None, None, None)
    assert T.ColorJitter(hue=0.5).hue == (-0.5, 0.5)


@pytest.mark.parametrize("kwargs", [
    {"brightness": -0.1}, {"contrast": -1}, {"saturation": -0.5}, {"hue": -0.1},  # negative numbers
    {"hue": 0.6},                                                                    # hue number above 0.5
    {"brightness": (1.2, 0.8)}, {"hue": (0.1, -0.1)},                                # unordered pairs
    {"contrast": (-0.1, 1.0)}, {"saturation": (-1, 0)},                              # pairs below 0
    {"hue": (-0.6, 0.0)}, {"hue": (0.0, 0.51)},                                      # hue pairs outside [-0.5, 0.5]
    {"brightness": (0.5, 1.0, 1.5)}, {"contrast": "0.2"}, {"saturation": None}, {"hue": (0.1,)},
    {"brightness": ("a", "b")},
    {"value_range": 0.0}, {"value_range": -1.0},
])
def test_bad_parameters_raise_value_error(kwargs):
    with pytest.raises(ValueError):
        T.ColorJitter(**kwargs)


# ------------------------------------------------------------------ augmentation_loader
def _config(aug):
    return SimpleNamespace(augmentation=aug)


def test_augmentation_loader_builds_color_jitter_in_key_order():
    """Fails with NotImplementedError without the feature."""
    ra = T.augmentation_loader(_config({
        "p": 0.5,
        "GaussianBlur": {"kernel_size": "5, 9", "sigma": "0.1, 5"},
        "RandomHorizontalFlip": {"p": 0.5},
        "ColorJitter": {"brightness": 0.2, "contrast": 0.2, "saturation": 0.2, "hue": 0.1},
    }), 0.5)
    assert ra.p == 0.5
    blur, flip, cj = ra.transforms
    assert isinstance(blur, T.GaussianBlur) and blur.kernel_size == (5, 9) and blur.sigma == (0.1, 5.0)
    assert isinstance(flip, T.RandomHorizontalFlip) and flip.p == 0.5
    assert isinstance(cj, T.ColorJitter)
    assert cj.brightness == pytest.approx((0.8, 1.2)) and cj.contrast == pytest.approx((0.8, 1.2))
    assert cj.saturation == pytest.approx((0.8, 1.2)) and cj.hue == pytest.approx((-0.1, 0.1))
    assert cj.value_range == 255.0


def test_augmentation_loader_color_jitter_first():
    ra = T.augmentation_loader(_config({
        "p": 0.5,
        "ColorJitter": {"brightness": [0.5, 1.5], "contrast": 0, "saturation": 0.3, "hue": 0},
        "GaussianBlur": {"kernel_size": "3", "sigma": "1, 2"},
    }), 0.25)
    cj, blur = ra.transforms
    assert isinstance(cj, T.ColorJitter) and isinstance(blur, T.GaussianBlur)
    assert cj.brightness == (0.5, 1.5) and cj.contrast is None and cj.hue is None
    assert cj.saturation == pytest.approx((0.7, 1.3))
    assert ra.p == 0.25


def test_random_brightness_variant_still_raises():
    with pytest.raises(NotImplementedError):
        T.augmentation_loader(_config({"p": 0.5, "ColorJitterWithRandomBrightness": {"brightness": 0.2}}), 0.5)


def test_shipped_config_with_the_block_uncommented(tmp_path):
    """The ColorJitter block of rtsds_amd/config.yaml is the reference's, commented out;
    uncommented it loads into a ColorJitter behind the two default augmentations."""
    text = open(os.path.join(os.path.dirname(T.__file__), "config.yaml")).read()
    block = ["  # ColorJitter:", "  #   brightness: 0.2", "  #   contrast: 0.2", "  #   saturation: 0.2",
             "  #   hue: 0.1"]
    lines = text.split("\n")
    at = lines.index(block[0])
    assert lines[at:at + 5] == block
    lines[at:at + 5] = [ln.replace("# ", "", 1) for ln in block]
    aug = yaml.safe_load("\n".join(lines))["augmentation"]
    ra = T.augmentation_loader(_config(aug), 0.5)
    assert [type(t) for t in ra.transforms] == [T.GaussianBlur, T.RandomHorizontalFlip, T.ColorJitter]
    assert ra.transforms[2].hue == pytest.approx((-0.1, 0.1))


# ------------------------------------------------------------------ draw order
def _draws(ranges):
    """get_params restated: the permutation, then one uniform per enabled op in b, c, s, h order."""
    order = tuple(torch.randperm(4).tolist())
    return (order,) + tuple(None if r is None else float(torch.empty(1).uniform_(r[0], r[1])) for r in ranges)


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_params_draw_order_all_on(seed):
    cj = T.ColorJitter(brightness=0.4, contrast=(0.5, 1.5), saturation=0.3, hue=0.2)
    torch.manual_seed(seed)
    got = cj.params()
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    want = _draws([(0.6, 1.4), (0.5, 1.5), (0.7, 1.3), (-0.2, 0.2)])
    assert got == want
    assert torch.equal(state, torch.get_rng_state())
    assert sorted(got[0]) == [0, 1, 2, 3] and all(isinstance(i, int) for i in got[0])
    assert 0.6 <= got[1] <= 1.4 and 0.5 <= got[2] <= 1.5 and 0.7 <= got[3] <= 1.3 and -0.2 <= got[4] <= 0.2


@pytest.mark.parametrize("seed", [0, 3])
def test_params_draw_order_hue_and_contrast_only(seed):
    cj = T.ColorJitter(contrast=0.5, hue=(-0.5, 0.5))
    torch.manual_seed(seed)
    got = cj.params()
    torch.manual_seed(seed)
    want = _draws([None, (0.5, 1.5), None, (-0.5, 0.5)])
    assert got == want
    assert got[1] is None and got[3] is None and got[2] is not None and got[4] is not None


def test_decisions_sequence_coin_sigma_flip_permutation_factors():
    blur = T.GaussianBlur((5, 9), (0.1, 5.0))
    cj = T.ColorJitter(0.2, 0.2, 0.2, 0.1)
    ra = T.RandomApply([blur, T.RandomHorizontalFlip(0.5), cj], p=1.0)
    torch.manual_seed(11)
    ops, flip = T._decisions(ra)
    state = torch.get_rng_state()
    torch.manual_seed(11)
    torch.rand(1)                                                # RandomApply's coin
    sigma = float(torch.empty(1).uniform_(0.1, 5.0))            # GaussianBlur.get_params
    want_flip = bool(torch.rand(1) < 0.5)                        # the flip's coin
    want = _draws([(0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1)])
    assert torch.equal(state, torch.get_rng_state())
    assert flip == want_flip
    assert [t for t, _ in ops] == [blur, cj]
    assert ops[0][1] == sigma and ops[1][1] == want


def test_decisions_color_jitter_first():
    blur = T.GaussianBlur(3, (0.5, 1.0))
    cj = T.ColorJitter(hue=0.3)
    ra = T.RandomApply([cj, blur], p=1.0)
    torch.manual_seed(5)
    ops, flip = T._decisions(ra)
    torch.manual_seed(5)
    torch.rand(1)
    want = _draws([None, None, None, (-0.3, 0.3)])
    sigma = float(torch.empty(1).uniform_(0.5, 1.0))
    assert flip is False
    assert [t for t, _ in ops] == [cj, blur] and ops[0][1] == want and ops[1][1] == sigma


def test_decisions_without_color_jitter_draw_what_they_drew_before():
    """Blur + flip: coin, sigma, flip coin and nothing else; the coin alone when it fails."""
    ra = T.RandomApply([T.GaussianBlur((5, 9), (0.1, 5.0)), T.RandomHorizontalFlip(0.5)], p=1.0)
    torch.manual_seed(2)
    ops, flip = T._decisions(ra)
    state = torch.get_rng_state()
    torch.manual_seed(2)
    torch.rand(1)
    sigma = float(torch.empty(1).uniform_(0.1, 5.0))
    want_flip = bool(torch.rand(1) < 0.5)
    assert torch.equal(state, torch.get_rng_state())
    assert len(ops) == 1 and ops[0][1] == sigma and flip == want_flip
    ra.p = 0.0
    torch.manual_seed(2)
    assert T._decisions(ra) == ([], False)
    state = torch.get_rng_state()
    torch.manual_seed(2)
    torch.rand(1)
    assert torch.equal(state, torch.get_rng_state())
    assert T._decisions(None) == ([], False)


# ------------------------------------------------------------------ C entry point
OK, SHAPE, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4


def _call(**over):
    """rtsds_color_jitter with valid arguments except those overridden; the pointers are dummies
    (validation returns before anything is launched or dereferenced on the device)."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    a = dict(src=p, src_u8=1, dst=p, c=3, h=2, w=2, order=(0, 1, 2, 3), mask=15, fb=1.0, fc=1.0, fs=1.0, fh=0.0,
             bound=255.0, ws=None, ws_bytes=0, stream=None)
    a.update(over)
    order = (ctypes.c_int * 4)(*a["order"]) if a["order"] is not None else None
    rc = _lib.load().rtsds_color_jitter(a["src"], a["src_u8"], a["dst"], a["c"], a["h"], a["w"], order, a["mask"],
                                        a["fb"], a["fc"], a["fs"], a["fh"], a["bound"], a["ws"], a["ws_bytes"],
                                        a["stream"])
    del buf
    return rc


@pytest.mark.parametrize("over", [
    {"h": 0}, {"w": -1}, {"c": 0}, {"src": None}, {"dst": None}, {"order": None},
    {"order": (0, 1, 2, 2)}, {"order": (0, 1, 2, 4)}, {"order": (-1, 0, 1, 2)},
    {"fh": 0.51}, {"fh": -0.6}, {"fh": float("nan")}, {"fb": -0.1}, {"fc": -1.0}, {"fs": -1e-3},
    {"bound": 0.0}, {"bound": -255.0}, {"mask": 16}, {"mask": -1},
])
def test_entry_point_rejects_bad_arguments(over):
    assert _call(**over) == SHAPE


@pytest.mark.parametrize("c", [1, 4])
def test_entry_point_needs_three_channels(c):
    assert _call(c=c) == UNSUPPORTED


def test_entry_point_needs_a_workspace_for_contrast():
    lib = _lib.load()
    need = lib.rtsds_color_jitter_workspace(2, 2)
    assert need > 0
    buf = ctypes.create_string_buffer(int(need))
    assert _call(ws=None, ws_bytes=need) == WORKSPACE
    assert _call(ws=ctypes.addressof(buf), ws_bytes=need - 1) == WORKSPACE
    assert _call(mask=2, ws=None, ws_bytes=0) == WORKSPACE
    # bad shapes are reported before the workspace
    assert _call(h=0, ws=None) == SHAPE and _call(c=4, ws=None) == UNSUPPORTED


def test_workspace_query():
    lib = _lib.load()
    assert lib.rtsds_color_jitter_workspace(0, 5) == 0 and lib.rtsds_color_jitter_workspace(5, -1) == 0
    small, gta = lib.rtsds_color_jitter_workspace(1, 1), lib.rtsds_color_jitter_workspace(1052, 1914)
    assert 0 < small <= gta <= 1 << 16  # a capped grid of partials, not a function of the image size
    assert lib.rtsds_color_jitter_workspace(4000, 4000) == gta


# ------------------------------------------------------------------ premises of the GPU parity tests
@pytest.mark.parametrize("name", sorted(R.SETS))
def test_reference_sets_stay_off_the_clamps(name):
    """At most 25 % of the fp64 outputs of sets 1-3 sit on a clamp in any of the 24 orders
    (otherwise the clamp would hide errors); the saturating set has no cap."""
    img = R.parity_image()
    worst = 0.0
    for order in R.ORDERS:
        ref, _ = R.refs(img, order, R.SETS[name])
        worst = max(worst, ((ref <= 0) | (ref >= 255.0)).double().mean().item())
    print(f"{name}: worst clamped share {worst:.3f}")
    assert worst <= 0.25


def test_reference_is_scale_homogeneous_and_identity_when_off():
    img = R.parity_image().double()
    assert torch.equal(R.color_jitter(img, (0, 1, 2, 3), None, None, None, None), img)
    a = R.color_jitter(img, (2, 0, 1, 3), *R.SETS["set1"], bound=255.0)
    b = R.color_jitter(img / 255.0, (2, 0, 1, 3), *R.SETS["set1"], bound=1.0) * 255.0
    assert (a - b).abs().max().item() < 1e-9
    # hue by a whole turn is the identity up to rounding
    c = R.hue(img, 0.5, 255.0)
    assert (R.hue(c, 0.5, 255.0) - img).abs().max().item() < 1e-9
