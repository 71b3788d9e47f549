"""Fourier Domain Adaptation without a GPU: the premises and the pinned tolerances of the GPU parity
tests (tests/fda_ref.py, tests/pinned/fda_tol.json), parameter handling, the config loader, the
order of the draws from torch's CPU generator, and the argument validation of rtsds_fda_workspace /
rtsds_fda_spectrum / rtsds_fda_apply (which comes before any HIP call)."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

from rtsds_amd import _lib
from rtsds_amd import transforms as T

from tests import fda_ref as R

PINNED = json.load(open(os.path.join(os.path.dirname(__file__), "pinned", "fda_tol.json")))
IDS = [R.key(*s) for s in R.SHAPES]
case, spectrum_errors = R.case, R.spectrum_errors  # per shape, computed once and shared with the GPU tests


# ------------------------------------------------------------------ premises
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_band_identity_equals_the_published_formulation(shape):
    c = case(*shape)
    err = float(np.abs(c.out64 - c.oracle).max())
    print(f"{R.key(*shape)}: max |apply_band fp64 - fda_fft| = {err:.3e}")
    assert err <= 1e-9
    assert max(spectrum_errors(c.s64, np.abs(c.s64) / (shape[0] * shape[1]), c.band, shape[0], shape[1])) <= 1e-12


@pytest.mark.parametrize("strength", [0.0, 0.5])
def test_blend_identity(strength):
    h, w, b = 37, 53, 3
    c = case(h, w, b)
    out = R.apply_band(c.src, c.s64, c.t64, b, strength)
    assert float(np.abs(out - R.fda_fft(c.src, c.tgt, b, strength)).max()) <= 1e-9
    if strength == 0.0:
        assert np.array_equal(out, c.src.astype(np.float64))


def test_target_of_another_size_agrees_on_equal_sizes_only():
    """The bank stores |F| / (hw), so a target of the source's size gives the published result; a
    target of another size is defined by the band formula alone (no FFT statement to compare with)."""
    src = R.source(64, 96)
    same, other = R.reference(64, 96), R.reference(37, 53)
    s, _ = R.band_spectrum(src, 2)
    assert float(np.abs(R.apply_band(src, s, R.band_spectrum(same, 2)[1], 2) - R.fda_fft(src, same, 2)).max()) <= 1e-9
    out = R.apply_band(src, s, R.band_spectrum(other, 2)[1], 2)
    assert np.isfinite(out).all() and float(np.abs(out - src).mean()) >= 5.0
    # the mean moves to the target's own mean, whatever its size
    assert np.allclose(out.mean((0, 1)), other.mean((0, 1)), atol=1e-9)


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_the_pairs_move_stay_in_range_and_have_no_vanishing_coefficient(shape):
    h, w, b = shape
    c = case(*shape)
    moved = float(np.abs(c.oracle - c.src).mean())
    outside = float(((c.oracle < 0) | (c.oracle > 255)).mean())
    floor = R.band_floor(c.src, b)
    print(f"{R.key(*shape)}: mean |out - src| {moved:.1f}, outside [0, 255] {outside:.4f}, min / median amplitude {floor:.4f}")
    assert moved >= 5.0 and outside < 0.05 and floor >= 1e-3


def test_other_test_sources_have_no_vanishing_coefficient():
    assert R.band_floor(R.source(), 2) >= 1e-3 and R.band_floor(R.reference(), 3) >= 1e-3
    assert R.band_floor(R.noise(64, 96), 2) >= 1e-3


# ------------------------------------------------------------------ tolerances
def test_pinned_file_lists_exactly_the_test_shapes():
    assert sorted(PINNED) == sorted(IDS + [k + "_spectrum" for k in IDS])


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_fp32_restatement_stays_within_the_pinned_error(shape):
    h, w, b = shape
    c = case(*shape)
    err = float(np.abs(c.out32.astype(np.float64) - c.oracle).max())
    e_spec, e_amp = spectrum_errors(c.s32.astype(np.complex128), c.a32.astype(np.float64), c.band, h, w)
    diff = np.abs(R.to_u8(c.out32).astype(np.int64) - R.to_u8(c.oracle).astype(np.int64))
    print(f"{R.key(*shape)}: fp32 apply {err:.3e} (pinned {PINNED[R.key(*shape)]:.1e}), spectrum {e_spec:.3e} / amplitude "
          f"{e_amp:.3e} (pinned {PINNED[R.key(*shape) + '_spectrum']:.1e}), uint8 off by one at {(diff > 0).mean():.2e}")
    assert err <= PINNED[R.key(*shape)]
    assert max(e_spec, e_amp) <= PINNED[R.key(*shape) + "_spectrum"]
    assert diff.max() <= 1 and (diff > 0).mean() <= 1e-3


# ------------------------------------------------------------------ parameters
class StubBank:
    """len(), b and amp(k), nothing on a device."""

    def __init__(self, n, b=None):
        self.n = n
        if b is not None:
            self.b = b

    def __len__(self):
        return self.n

    def amp(self, k):
        return ("amp", k)


def test_defaults_and_pairs():
    bank = StubBank(3)
    fa = T.FourierAdaptation(bank)
    assert fa.bank is bank and fa.p == 0.5 and fa.beta == 0.01 and fa.strength == (1.0, 1.0)
    fa = T.FourierAdaptation(bank, p=1, beta=0.05, strength=[0.25, 0.75])
    assert fa.p == 1.0 and fa.beta == 0.05 and fa.strength == (0.25, 0.75)
    assert T.FourierAdaptation(bank, strength=0.5).strength == (0.5, 0.5)


@pytest.mark.parametrize("kwargs", [
    {"p": -0.1}, {"p": 1.5}, {"p": None}, {"p": "0.5"}, {"p": float("nan")}, {"p": True},
    {"beta": 0.0}, {"beta": 0.5}, {"beta": -0.01}, {"beta": 1}, {"beta": None}, {"beta": "0.01"}, {"beta": float("nan")},
    {"strength": (0.8, 0.2)}, {"strength": (-0.1, 0.5)}, {"strength": (0.5, 1.1)}, {"strength": (0.5,)},
    {"strength": (0.1, 0.2, 0.3)}, {"strength": "0.5, 1.0"}, {"strength": None}, {"strength": (float("nan"), 1.0)},
])
def test_bad_parameters_raise_value_error(kwargs):
    with pytest.raises(ValueError):
        T.FourierAdaptation(StubBank(1), **kwargs)


def test_band_arithmetic_and_limits():
    fa = T.FourierAdaptation(StubBank(1), beta=0.01)
    assert fa.band(720, 1280) == 7 and fa.band(1280, 720) == 7 and fa.band(1052, 1914) == 10
    assert fa.band(64, 96) == 1 and fa.band(3, 3) == 1          # floored at 1
    assert T.FourierAdaptation(StubBank(1), beta=0.05).band(720, 1280) == 36
    with pytest.raises(ValueError, match="limits"):
        fa.band(2, 9)                                           # 2b + 1 > min(h, w)
    with pytest.raises(ValueError, match="limits"):
        T.FourierAdaptation(StubBank(1), beta=0.1).band(700, 700)   # b = 70 > 64
    with pytest.raises(ValueError, match="limits"):
        fa.band(4097, 4096)                                     # h * w > 2^24
    assert T.FourierAdaptation(StubBank(1, b=7), beta=0.01).band(720, 1280) == 7
    with pytest.raises(ValueError, match="bank holds b = 7"):
        T.FourierAdaptation(StubBank(1, b=7), beta=0.01).band(1052, 1914)


# ------------------------------------------------------------------ draw order
@pytest.mark.parametrize("seed", [0, 1, 7])
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_params_consume_the_stream_histogram_matching_consumes(seed, p):
    fa = T.FourierAdaptation(StubBank(5), p=p, strength=(0.25, 0.75))
    hm = T.HistogramMatching(StubBank(5), p=p, strength=(0.25, 0.75))
    torch.manual_seed(seed)
    got = fa.params()
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    want = hm.params()
    assert torch.equal(state, torch.get_rng_state())
    assert (got is None) == (want is None)
    if got is not None:
        assert got[0] == want[0] and 0.25 <= got[1] <= 0.75 and T._strength_q8(got[1]) == want[1]
        assert isinstance(got[0], int) and isinstance(got[1], float)


def test_an_empty_bank_raises_only_when_taken():
    assert T.FourierAdaptation(StubBank(0), p=0.0).params() is None
    with pytest.raises(RuntimeError, match="empty"):
        T.FourierAdaptation(StubBank(0), p=1.0).params()


@pytest.mark.parametrize("first", [True, False])
def test_sample_draws_take_the_transform_at_its_position(first):
    blur = T.GaussianBlur((5, 9), (0.1, 5.0))
    flip_t = T.RandomHorizontalFlip(0.5)
    fa = T.FourierAdaptation(StubBank(6), p=1.0, strength=(0.5, 1.0))
    ra = T.RandomApply([fa, blur, flip_t] if first else [blur, flip_t, fa], p=1.0)
    torch.manual_seed(11)
    ops, flip, window, flip_label, style, spectral = T._sample_draws_all(ra, 8, 8)
    state = torch.get_rng_state()
    torch.manual_seed(11)
    torch.rand(1)                                                # RandomApply's coin
    if first:
        want = fa.params()
    sigma = float(torch.empty(1).uniform_(0.1, 5.0))
    want_flip = bool(torch.rand(1) < 0.5)
    if not first:
        want = fa.params()
    assert torch.equal(state, torch.get_rng_state())
    assert spectral == (fa,) + want and style is None
    assert [t for t, _ in ops] == [blur] and ops[0][1] == sigma and flip == want_flip
    # the narrower helpers keep their arity and their draws
    torch.manual_seed(11)
    assert T._sample_draws_styled(ra, 8, 8) == (ops, flip, None, False, None)
    assert torch.equal(state, torch.get_rng_state())
    torch.manual_seed(11)
    assert T._sample_draws(ra, 8, 8) == (ops, flip, None, False) and T._decisions(ra) is not None


def test_lists_without_the_transform_draw_what_they_drew_before():
    """The state of the generator after _sample_draws_styled equals that after the draws the list
    made before the class existed, restated here."""
    hm = T.HistogramMatching(StubBank(4), p=1.0, strength=(0.5, 1.0))
    ra = T.RandomApply([T.GaussianBlur((5, 9), (0.1, 5.0)), hm, T.RandomHorizontalFlip(0.5)], p=1.0)
    torch.manual_seed(2)
    got = T._sample_draws_all(ra, 8, 8)
    state = torch.get_rng_state()
    torch.manual_seed(2)
    torch.rand(1)
    sigma = float(torch.empty(1).uniform_(0.1, 5.0))
    style = hm.params()
    want_flip = bool(torch.rand(1) < 0.5)
    assert torch.equal(state, torch.get_rng_state())
    assert got[5] is None and got[4] == (hm.bank,) + style and got[0][0][1] == sigma and got[1] == want_flip
    torch.manual_seed(2)
    assert T._sample_draws_styled(ra, 8, 8) == got[:5]
    assert torch.equal(state, torch.get_rng_state())
    ra.p = 0.0
    assert T._sample_draws_all(ra) == ([], False, None, False, None, None)
    assert T._sample_draws_all(None) == ([], False, None, False, None, None)


# ------------------------------------------------------------------ augmentation_loader
def _config(aug):
    return SimpleNamespace(augmentation=aug)


def test_augmentation_loader_builds_the_transform_in_key_order_with_its_bank():
    hists, amps = object(), StubBank(4, b=7)
    ra = T.augmentation_loader(_config({
        "p": 0.5,
        "GaussianBlur": {"kernel_size": "5, 9", "sigma": "0.1, 5"},
        "FourierAdaptation": {"p": 0.25, "beta": 0.02, "strength": "0.5, 1.0", "bank": 8},
        "HistogramMatching": {"p": 0.5},
    }), 0.5, bank=hists, spectrum_bank=amps)
    blur, fa, hm = ra.transforms
    assert isinstance(blur, T.GaussianBlur) and isinstance(hm, T.HistogramMatching) and hm.bank is hists
    assert isinstance(fa, T.FourierAdaptation) and fa.bank is amps
    assert fa.p == 0.25 and fa.beta == 0.02 and fa.strength == (0.5, 1.0)
    (fa,) = T.augmentation_loader(_config({"p": 0.5, "FourierAdaptation": {"strength": 0.5}}), 0.5, spectrum_bank=amps).transforms
    assert fa.p == 0.5 and fa.beta == 0.01 and fa.strength == (0.5, 0.5)


def test_augmentation_loader_raises_without_a_spectrum_bank():
    cfg = _config({"p": 0.5, "FourierAdaptation": {"p": 0.5}})
    with pytest.raises(RuntimeError, match="bank"):
        T.augmentation_loader(cfg, 0.5)
    with pytest.raises(RuntimeError, match="bank"):
        T.augmentation_loader(cfg, 0.5, bank=object())           # the histogram bank is not it
    with pytest.raises(TypeError):
        T.augmentation_loader(cfg, 0.5, None, StubBank(1))       # keyword only


def test_shipped_config_carries_the_commented_key():
    text = open(os.path.join(os.path.dirname(T.__file__), "config.yaml")).read()
    assert "FourierAdaptation" not in yaml.safe_load(text)["augmentation"]
    lines = text.split("\n")
    at = lines.index("  # FourierAdaptation: {p: 0.5, beta: 0.01, strength: \"0.5, 1.0\", bank: 64}")
    lines[at] = lines[at].replace("# ", "", 1)
    aug = yaml.safe_load("\n".join(lines))["augmentation"]
    ra = T.augmentation_loader(_config(aug), 0.5, spectrum_bank=StubBank(2, b=7))
    fa = ra.transforms[-1]
    assert isinstance(fa, T.FourierAdaptation) and fa.strength == (0.5, 1.0) and fa.band(720, 1280) == 7
    assert aug["FourierAdaptation"]["bank"] == 64


def test_python_layer_refuses_host_tensors():
    img = torch.zeros((8, 8, 3), dtype=torch.uint8)
    spec, amp = torch.zeros((3, 3, 2, 2)), torch.zeros((3, 3, 2))
    with pytest.raises(RuntimeError, match="HIP"):
        T.band_spectrum(img, 1)
    with pytest.raises(RuntimeError, match="HIP"):
        T.fourier_adapt(img, spec, amp)
    with pytest.raises(RuntimeError, match="uint8"):
        T.band_spectrum(img.float(), 1)
    with pytest.raises(ValueError):
        T.SpectrumBank(0, 7, device="cpu")
    with pytest.raises(ValueError):
        T.SpectrumBank(4, 65, device="cpu")


# ------------------------------------------------------------------ C entry points
OK, SHAPE, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
_BUF = ctypes.create_string_buffer(4096 + 16)
_PTR = (ctypes.addressof(_BUF) + 15) & ~15  # dummies: validation returns before anything is dereferenced


def _spectrum(**over):
    a = dict(img=_PTR, c=3, h=16, w=16, b=2, spec=_PTR, amp=_PTR, ws=_PTR, ws_bytes=1 << 30, stream=None)
    a.update(over)
    return _lib.load().rtsds_fda_spectrum(a["img"], a["c"], a["h"], a["w"], a["b"], a["spec"], a["amp"], a["ws"],
                                          a["ws_bytes"], a["stream"])


def _apply(**over):
    a = dict(src=_PTR, dst=_PTR, dst_u8=1, c=3, h=16, w=16, b=2, spec=_PTR, amp=_PTR, strength=1.0, stream=None)
    a.update(over)
    return _lib.load().rtsds_fda_apply(a["src"], a["dst"], a["dst_u8"], a["c"], a["h"], a["w"], a["b"], a["spec"],
                                       a["amp"], a["strength"], a["stream"])


def test_workspace_query():
    ws = _lib.load().rtsds_fda_workspace
    assert ws(720, 1280, 7) == 720 * 3 * 8 * 8 and ws(3, 3, 1) > 0 and ws(130, 134, 64) > 0
    assert ws(16, 16, 0) == 0 and ws(4, 16, 2) == 0


BAD_SHAPES = [{"b": 0}, {"b": 65, "h": 256, "w": 256}, {"b": 8}, {"h": 4, "w": 64}, {"h": 64, "w": 4}, {"h": 4097, "w": 4096},
              {"h": 0}, {"w": -1}, {"c": 0}]


@pytest.mark.parametrize("over", BAD_SHAPES + [{"img": None}, {"spec": None, "amp": None}])
def test_spectrum_entry_rejects_bad_arguments(over):
    assert _spectrum(**over) == SHAPE


@pytest.mark.parametrize("over", BAD_SHAPES + [{"src": None}, {"dst": None}, {"spec": None}, {"amp": None}, {"strength": 1.5},
                                               {"strength": -0.01}, {"strength": float("nan")}])
def test_apply_entry_rejects_bad_arguments(over):
    assert _apply(**over) == SHAPE


@pytest.mark.parametrize("c", [1, 4])
def test_entries_need_three_channels(c):
    assert _spectrum(c=c) == UNSUPPORTED and _apply(c=c) == UNSUPPORTED
    assert _spectrum(c=c, b=0) == SHAPE and _apply(c=c, strength=1.5) == SHAPE   # a bad shape is reported first


def test_entries_need_aligned_fp32_pointers_and_a_workspace():
    assert _spectrum(spec=_PTR + 2) == UNSUPPORTED and _spectrum(amp=_PTR + 1) == UNSUPPORTED
    assert _apply(spec=_PTR + 1) == UNSUPPORTED and _apply(amp=_PTR + 2) == UNSUPPORTED
    assert _apply(dst_u8=0, dst=_PTR + 2) == UNSUPPORTED
    need = _lib.load().rtsds_fda_workspace(16, 16, 2)
    assert _spectrum(ws_bytes=need - 1) == WORKSPACE and _spectrum(ws=None) == WORKSPACE
