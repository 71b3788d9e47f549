"""Fourier Domain Adaptation on the device (rtsds_amd.transforms: band_spectrum, fourier_adapt,
SpectrumBank, FourierAdaptation in the ImagePipeline; csrc/fda.hip) against the published fft2 /
fftshift formulation in fp64 (tests/fda_ref.py: fda_fft).  The tolerances are 8 x the error of the
fp32 numpy restatement of the kernels' formulas at the same shape (tests/pinned/fda_tol.json; the
margin covers a summation order other than numpy's and the hardware's sincos); the premises -- the
band identity, pairs that move, no vanishing coefficient -- are checked in tests/test_fda_cpu.py.

Shapes: 3x3 b=1 the band is the whole spectrum; 5x7 b=2 odd sizes, tails only; 64x96 b=2 whole
groups of four pixels on an aligned base (the dword path); 37x53 b=3 odd sizes, where the fftshift
centre matters; 67x131 b=5 an odd tail and more than one tile of rows; 130x134 b=64 the largest
band, one short of Nyquist; 720x1280 b=7 the real frame, where the capped grids make more than one
pass and a row spans two tiles of columns."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from rtsds_amd import transforms as T  # noqa: E402

from tests import fda_ref as R  # noqa: E402

DEV = "cuda"
MARGIN = 8.0
PINNED = json.load(open(os.path.join(os.path.dirname(__file__), "pinned", "fda_tol.json")))
IDS = [R.key(*s) for s in R.SHAPES]
SIZE = (24, 40)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _offset_by_one(a):
    """The image on the device with its base one byte past an aligned allocation."""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.zeros(flat.numel() + 17, dtype=torch.uint8, device=DEV)
    buf[1:1 + flat.numel()] = flat.to(DEV)
    view = buf[1:1 + flat.numel()].view(a.shape)
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    return view


def _complex(spec):
    s = spec.cpu().numpy().astype(np.float64)
    return s[..., 0] + 1j * s[..., 1]


def _band_of(img, b):
    """(spec, amp_norm) of the device for a numpy image, as device tensors."""
    return T.band_spectrum(_dev(img), b)


def _amp_dev(amp):
    return torch.from_numpy(np.ascontiguousarray(amp, dtype=np.float32)).to(DEV)


def _u8_close(got, oracle):
    """|got - rint(oracle)| <= 1 everywhere, off at no more than 1e-3 of the pixels."""
    diff = np.abs(got.cpu().numpy().astype(np.int64) - R.to_u8(oracle).astype(np.int64))
    share = float((diff > 0).mean())
    print(f"uint8: max difference {diff.max()}, share off by one {share:.2e}")
    return diff.max() <= 1 and share <= 1e-3


# ------------------------------------------------------------------ spectrum
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_spectrum_against_fft2(shape):
    h, w, b = shape
    c = R.case(*shape)
    spec, amp = _band_of(c.src, b)
    assert spec.dtype == torch.float32 and tuple(spec.shape) == (3, 2 * b + 1, b + 1, 2)
    assert amp.dtype == torch.float32 and tuple(amp.shape) == (3, 2 * b + 1, b + 1)
    e_spec, e_amp = R.spectrum_errors(_complex(spec), amp.cpu().numpy().astype(np.float64), c.band, h, w)
    tol = MARGIN * PINNED[R.key(*shape) + "_spectrum"]
    print(f"{R.key(*shape)}: spectrum {e_spec:.3e}, amplitude {e_amp:.3e}, tolerance {tol:.3e}")
    assert e_spec <= tol and e_amp <= tol


def test_spectrum_fills_given_tensors_and_is_reproducible():
    img = _dev(R.source(67, 131))
    spec = torch.full((3, 11, 6, 2), 7.0, device=DEV)
    amp = torch.full((3, 11, 6), 7.0, device=DEV)
    s, a = T.band_spectrum(img, 5, spec=spec, amp=amp)
    assert s is spec and a is amp
    s2, a2 = T.band_spectrum(img, 5)
    assert torch.equal(s, s2) and torch.equal(a, a2)
    # the mirror half: F(-u, 0) = conj F(u, 0), to rounding
    z = _complex(s)
    assert np.abs(z[:, ::-1, 0] - np.conj(z[:, :, 0])).max() <= 1e-6 * np.abs(z).max()


@pytest.mark.parametrize("h,w,b", [(64, 96, 2), (67, 131, 5)], ids=["dword_path", "byte_path"])
def test_spectrum_of_an_unaligned_base_has_the_same_bits(h, w, b):
    src = R.case(h, w, b).src
    s0, a0 = _band_of(src, b)
    s1, a1 = T.band_spectrum(_offset_by_one(src), b)
    assert torch.equal(s0, s1) and torch.equal(a0, a1)


# ------------------------------------------------------------------ apply
def _adapt(shape, dtype, strength=1.0, src_dev=None, out=None):
    h, w, b = shape
    c = R.case(*shape)
    x = _dev(c.src) if src_dev is None else src_dev
    spec, _ = T.band_spectrum(x, b)
    _, amp_t = _band_of(c.tgt, b)
    return T.fourier_adapt(x, spec, amp_t, strength, out=out, dtype=dtype)


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_apply_fp32_against_the_oracle(shape):
    c = R.case(*shape)
    got = _adapt(shape, torch.float32)
    assert got.dtype == torch.float32 and tuple(got.shape) == c.src.shape
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - np.clip(c.oracle, 0, 255)).max())
    tol = MARGIN * PINNED[R.key(*shape)]
    print(f"{R.key(*shape)}: max |out - fda_fft| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_apply_uint8_against_the_oracle(shape):
    c = R.case(*shape)
    got = _adapt(shape, torch.uint8)
    assert got.dtype == torch.uint8 and tuple(got.shape) == c.src.shape
    assert _u8_close(got, c.oracle)


def test_apply_clamps():
    """A bright target on a bright source leaves [0, 255] in the oracle: both epilogues clamp."""
    h, w, b = 37, 53, 3
    src = R.reference(h, w, seed=11)
    tgt = np.clip(R.reference(h, w, seed=12).astype(np.int64) + 90, 0, 255).astype(np.uint8)
    oracle = R.fda_fft(src, tgt, b)
    assert (oracle > 255).mean() > 0.05
    x = _dev(src)
    spec, _ = T.band_spectrum(x, b)
    _, amp_t = _band_of(tgt, b)
    f = T.fourier_adapt(x, spec, amp_t, dtype=torch.float32).cpu().numpy().astype(np.float64)
    assert f.max() == 255.0 and float(np.abs(f - np.clip(oracle, 0, 255)).max()) <= MARGIN * PINNED[R.key(h, w, b)]
    assert _u8_close(T.fourier_adapt(x, spec, amp_t), oracle)


@pytest.mark.parametrize("strength", [0.5, 0.25])
def test_blend(strength):
    shape = (37, 53, 3)
    c = R.case(*shape)
    oracle = R.fda_fft(c.src, c.tgt, 3, strength)
    got = _adapt(shape, torch.float32, strength)
    assert float(np.abs(got.cpu().numpy().astype(np.float64) - np.clip(oracle, 0, 255)).max()) <= MARGIN * PINNED[R.key(*shape)]
    assert _u8_close(_adapt(shape, torch.uint8, strength), oracle)


# ------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("shape", [(5, 7, 2), (64, 96, 2), (67, 131, 5)], ids=lambda s: R.key(*s))
def test_strength_zero_returns_the_source_bit_for_bit(shape):
    c = R.case(*shape)
    assert torch.equal(_adapt(shape, torch.uint8, 0.0).cpu(), torch.from_numpy(c.src))
    assert torch.equal(_adapt(shape, torch.float32, 0.0).cpu(), torch.from_numpy(c.src.astype(np.float32)))


@pytest.mark.parametrize("shape", [(37, 53, 3), (64, 96, 2), (130, 134, 64)], ids=lambda s: R.key(*s))
def test_target_equal_to_the_source_returns_the_source(shape):
    h, w, b = shape
    c = R.case(*shape)
    x = _dev(c.src)
    spec, amp = T.band_spectrum(x, b)
    assert torch.equal(T.fourier_adapt(x, spec, amp).cpu(), torch.from_numpy(c.src))
    f = T.fourier_adapt(x, spec, amp, dtype=torch.float32).cpu().numpy().astype(np.float64)
    assert float(np.abs(f - c.src).max()) <= MARGIN * PINNED[R.key(*shape)]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("shape", [(64, 96, 2), (67, 131, 5)], ids=lambda s: R.key(*s))
def test_two_runs_give_equal_bits_and_an_unaligned_base_the_same(shape, dtype):
    c = R.case(*shape)
    a, b2 = _adapt(shape, dtype), _adapt(shape, dtype)
    assert torch.equal(a, b2)
    assert torch.equal(a, _adapt(shape, dtype, src_dev=_offset_by_one(c.src)))


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("shape", [(64, 96, 2), (67, 131, 5)], ids=lambda s: R.key(*s))
def test_in_place_equals_out_of_place(shape, unaligned):
    c = R.case(*shape)
    x = _offset_by_one(c.src) if unaligned else _dev(c.src)
    want = _adapt(shape, torch.uint8, src_dev=x)
    assert want is not x and torch.equal(x.cpu(), torch.from_numpy(c.src))   # the source is left as it was
    got = _adapt(shape, torch.uint8, src_dev=x, out=x)
    assert got is x and torch.equal(got, want)
    other = torch.empty_like(want)
    assert _adapt(shape, torch.uint8, src_dev=_dev(c.src), out=other) is other and torch.equal(other, want)


def test_fourier_adapt_refuses_what_it_cannot_do():
    x = _dev(R.source(16, 24))
    spec, amp = T.band_spectrum(x, 2)
    with pytest.raises(RuntimeError, match="in place"):
        T.fourier_adapt(x, spec, amp, out=x, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="strength"):
        T.fourier_adapt(x, spec, amp, 1.5)
    with pytest.raises(RuntimeError, match="amp_ref"):
        T.fourier_adapt(x, spec, amp[:, :, :2])
    with pytest.raises(RuntimeError, match="writes"):
        T.fourier_adapt(x, spec, amp, out=torch.empty((16, 24, 3), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="limits"):
        T.band_spectrum(x, 8)


# ------------------------------------------------------------------ target of another size
def test_target_of_another_size():
    src, tgt = R.source(64, 96), R.reference(37, 53)
    b = 2
    want = R.apply_band(src, R.band_spectrum(src, b)[0], R.band_spectrum(tgt, b)[1], b)
    assert float(np.abs(want - src).mean()) >= 5.0
    x = _dev(src)
    spec, _ = T.band_spectrum(x, b)
    _, amp_t = _band_of(tgt, b)
    got = T.fourier_adapt(x, spec, amp_t, dtype=torch.float32).cpu().numpy().astype(np.float64)
    assert float(np.abs(got - np.clip(want, 0, 255)).max()) <= MARGIN * PINNED[R.key(64, 96, 2)]
    assert _u8_close(T.fourier_adapt(x, spec, amp_t), want)


# ------------------------------------------------------------------ bank
REFS = [R.reference(37, 53, seed=21), R.reference(30, 44, seed=22), R.reference(64, 96, seed=23)]


def _bank(b=2, capacity=4):
    bank = T.SpectrumBank(capacity, b, DEV)
    bank.add([_dev(r) for r in REFS])
    return bank


def test_spectrum_bank_ring():
    bank = T.SpectrumBank(2, 2, DEV)
    assert len(bank) == 0 and bank.b == 2 and tuple(bank.data.shape) == (2, 3, 5, 3)
    with pytest.raises(IndexError):
        bank.amp(0)
    amps = [T.band_spectrum(_dev(r), 2)[1] for r in REFS]
    bank.add([_dev(REFS[0])])
    assert len(bank) == 1 and torch.equal(bank.amp(0), amps[0])
    with pytest.raises(IndexError):
        bank.amp(1)
    bank.add([_dev(REFS[1]), _dev(REFS[2])])                   # the third overwrites the oldest
    assert len(bank) == 2 and torch.equal(bank.amp(0), amps[2]) and torch.equal(bank.amp(1), amps[1])
    with pytest.raises(IndexError):
        bank.amp(2)
    with pytest.raises(IndexError):
        bank.amp(-1)
    with pytest.raises(ValueError, match="limits"):
        bank.add([_dev(R.noise(4, 40))])                        # the band does not fit


# ------------------------------------------------------------------ pipeline
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pipeline_equals_the_manual_chain(dtype):
    src = R.source(100, 150, seed=31)                            # beta = 0.02: b = 2
    blur, flip = T.GaussianBlur((5, 9), (0.1, 5.0)), T.RandomHorizontalFlip(0.5)
    bank = _bank()
    fa = T.FourierAdaptation(bank, p=1.0, beta=0.02, strength=(0.5, 1.0))
    with_t = T.ImagePipeline(SIZE, augment=T.RandomApply([blur, flip, fa], p=1.0))
    without = T.ImagePipeline(SIZE, augment=T.RandomApply([blur, flip], p=1.0))
    img = _dev(src)
    torch.manual_seed(5)
    got = with_t([img], dtype=dtype)
    state = torch.get_rng_state()
    assert torch.equal(img.cpu(), torch.from_numpy(src))        # the caller's image is unchanged
    torch.manual_seed(5)                                         # the draws, replayed by hand
    torch.rand(1)
    torch.empty(1).uniform_(0.1, 5.0)
    torch.rand(1)
    assert bool(torch.rand(1) < 1.0)
    k = int(torch.randint(0, 3, (1,)))
    s = float(torch.empty(1).uniform_(0.5, 1.0))
    assert torch.equal(state, torch.get_rng_state())
    assert with_t.last_spectral == [(k, s)] and with_t.last_style == [None] and 0.5 <= s <= 1.0
    adapted = T.fourier_adapt(img, T.band_spectrum(img, 2)[0], bank.amp(k), s)
    assert not torch.equal(adapted, img)
    torch.manual_seed(5)
    want = without([adapted], dtype=dtype)
    assert without.last_spectral == [None]
    assert got.dtype == dtype and torch.equal(got, want)
    torch.manual_seed(5)
    assert not torch.equal(got, without([img], dtype=dtype))    # and the adaptation did change the batch


def test_pipeline_with_both_style_keys_matches_histograms_first():
    src = R.source(100, 150, seed=32)
    hists = T.HistogramBank(4, DEV)
    hists.add([_dev(r) for r in REFS])
    bank = _bank()
    fa = T.FourierAdaptation(bank, p=1.0, beta=0.02)
    hm = T.HistogramMatching(hists, p=1.0)
    img = _dev(src)
    for order in ([fa, hm], [hm, fa]):                           # wherever the keys stand
        pipe = T.ImagePipeline(SIZE, augment=T.RandomApply(order, p=1.0))
        torch.manual_seed(3)
        got = pipe([img], dtype=torch.float32)
        (k, s), (kh, a) = pipe.last_spectral[0], pipe.last_style[0]
        assert torch.equal(img.cpu(), torch.from_numpy(src))
        matched = T.histogram_match(img, T.image_histogram(img), hists.hist(kh), a / 256.0)
        chained = T.fourier_adapt(matched, T.band_spectrum(matched, 2)[0], bank.amp(k), s)
        assert torch.equal(got, T.ImagePipeline(SIZE)([chained], dtype=torch.float32))
        swapped = T.fourier_adapt(img, T.band_spectrum(img, 2)[0], bank.amp(k), s)
        swapped = T.histogram_match(swapped, T.image_histogram(swapped), hists.hist(kh), a / 256.0)
        assert not torch.equal(got, T.ImagePipeline(SIZE)([swapped], dtype=torch.float32))


def test_pipeline_records_a_draw_per_sample_and_checks_the_band():
    bank = _bank()
    fa = T.FourierAdaptation(bank, p=0.5, beta=0.02)
    pipe = T.ImagePipeline(SIZE, augment=T.RandomApply([fa], p=1.0))
    imgs = [_dev(R.source(100 + i, 140, seed=40 + i)) for i in range(6)]
    torch.manual_seed(1)
    got = pipe(imgs, dtype=torch.float32)
    torch.manual_seed(1)
    want = []
    for _ in imgs:
        torch.rand(1)
        want.append(fa.params())
    assert pipe.last_spectral == want and pipe.last_style == [None] * 6
    assert any(d is None for d in want) and any(d is not None for d in want)
    plain = T.ImagePipeline(SIZE)
    for n, (img, d) in enumerate(zip(imgs, want)):
        if d is not None:
            img = T.fourier_adapt(img, T.band_spectrum(img, 2)[0], bank.amp(d[0]), d[1])
        assert torch.equal(got[n], plain([img], dtype=torch.float32)[0])
    with pytest.raises(ValueError, match="bank holds b = 2"):    # 200 x 300 at beta = 0.02 wants b = 4
        T.ImagePipeline(SIZE, augment=T.RandomApply([T.FourierAdaptation(bank, p=1.0, beta=0.02)], p=1.0))(
            [_dev(R.source(200, 300))], dtype=torch.float32)


# ------------------------------------------------------------------ wiring
def test_build_spectrum_bank_from_a_cityscapes_tree(tmp_path):
    from PIL import Image

    from rtsds_amd.datasets import CityScapes
    from rtsds_amd.main import build_spectrum_bank
    (tmp_path / "img" / "city").mkdir(parents=True)
    (tmp_path / "gt" / "city").mkdir(parents=True)
    rng = np.random.default_rng(40)
    for i in range(5):
        Image.fromarray(R.reference(16, 32, seed=50 + i)).save(tmp_path / "img" / "city" / f"city_{i:06d}_000019_leftImg8bit.png")
        Image.fromarray(rng.integers(0, 19, (16, 32), dtype=np.uint8)).save(
            tmp_path / "gt" / "city" / f"city_{i:06d}_000019_gtFine_labelTrainIds.png")
    ds = CityScapes(str(tmp_path / "gt"), str(tmp_path / "img"))
    bank = build_spectrum_bank(ds, 3, 2, DEV)
    idx = T.bank_indices(5, 3)
    assert idx == [0, 1, 3] and len(bank) == 3 and bank.b == 2
    for slot, i in enumerate(idx):
        assert torch.equal(bank.amp(slot), T.band_spectrum(ds[i][0].to(DEV), 2)[1])
    assert len(build_spectrum_bank(ds, 64, 2, DEV)) == 5        # a bank larger than the set holds the whole set
