"""Histogram matching on the device (rtsds_amd.transforms: image_histogram, histogram_match,
HistogramBank, HistogramMatching in the ImagePipeline; csrc/histmatch.hip) against the numpy
restatement tests/histmatch_ref.py.  Everything is integer, so every comparison is equality:
there are no tolerances.  The premises (the reference moves most values of the skewed pair, so
an identity kernel cannot pass) are checked in tests/test_histmatch_cpu.py."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from rtsds_amd import transforms as T  # noqa: E402

from tests import histmatch_ref as R  # noqa: E402

DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _hist_dev(h):
    """uint32 [3, 256] numpy -> the device tensor of the package's uint32 dtype."""
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int32)).to(DEV).view(T._U32)


def _same_hist(got, want):
    assert got.dtype == T._U32 and tuple(got.shape) == (3, 256)
    return torch.equal(got.view(torch.int32).cpu(), torch.from_numpy(np.ascontiguousarray(want).view(np.int32)))


def _offset_by_one(a):
    """The image on the device with its base one byte past an aligned allocation."""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.zeros(flat.numel() + 17, dtype=torch.uint8, device=DEV)
    buf[1:1 + flat.numel()] = flat.to(DEV)
    view = buf[1:1 + flat.numel()].view(a.shape)
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def _gta5():
    """(image, its histogram) at the GTA5 frame size: more than one pass of the capped grids."""
    img = R.source(*R.GTA5, seed=8)
    return img, R.histogram(img)


# ------------------------------------------------------------------ histogram
@pytest.mark.parametrize("h,w", [(1, 1), (1, 5),           # tails only (3 and 15 bytes)
                                 (3, 64), (64, 96),        # exact multiples of the 16-byte vector
                                 (67, 131)])               # odd tail
def test_histogram_sizes(h, w):
    img = R.noise(h, w, seed=h * 1000 + w)
    assert _same_hist(T.image_histogram(_dev(img)), R.histogram(img))


def test_histogram_gta5_size():
    img, want = _gta5()
    assert _same_hist(T.image_histogram(_dev(img)), want)


@pytest.mark.parametrize("name,img", [("noise", R.noise(67, 131)), ("constant", R.constant(67, 131)),
                                      ("two_valued", R.two_valued(67, 131)), ("sky", R.sky(67, 131)),
                                      ("ramp", R.ramp(5, 300))])
def test_histogram_contents(name, img):
    got = T.image_histogram(_dev(img))
    assert _same_hist(got, R.histogram(img))
    assert int(got.view(torch.int32).sum()) == img.size


def test_histogram_of_an_unaligned_base():
    img = R.sky(67, 131, seed=9)
    assert _same_hist(T.image_histogram(_offset_by_one(img)), R.histogram(img))


def test_histogram_overwrites_its_slot():
    a, b = R.noise(33, 47, seed=1), R.sky(20, 31, seed=2)
    out = torch.empty((3, 256), dtype=T._U32, device=DEV)
    assert T.image_histogram(_dev(a), out=out) is out
    assert _same_hist(out, R.histogram(a))
    T.image_histogram(_dev(b), out=out)
    assert _same_hist(out, R.histogram(b))


def test_histogram_is_reproducible():
    img = _dev(R.sky(67, 131, seed=3))
    a, b = T.image_histogram(img), T.image_histogram(img)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ match
def _check_match(src, hist_ref, a, *, dev_src=None, in_place=False):
    """histogram_match of src (strength a / 256) equals the reference, image and LUT."""
    hs = R.histogram(src)
    want, want_lut = R.match(src, hs, hist_ref, a)
    x = _dev(src) if dev_src is None else dev_src
    keep = x.clone()
    lut = torch.full((3, 256), 7, dtype=torch.uint8, device=DEV)
    got = T.histogram_match(x, _hist_dev(hs), _hist_dev(hist_ref), strength=a / 256.0, out=x if in_place else None,
                            lut=lut)
    assert got.dtype == torch.uint8 and got.shape == x.shape
    assert (got is x) == in_place
    assert torch.equal(lut.cpu(), torch.from_numpy(want_lut))
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    if not in_place:
        assert torch.equal(x, keep)  # the source is left as it was
    return want


def test_match_skewed_pair_of_different_sizes():
    src, ref = R.source(), R.reference()
    assert src.shape[:2] == (64, 96) and ref.shape[:2] == (37, 53)  # Ns != Nr: the cross-multiplication matters
    want = _check_match(src, R.histogram(ref), 256)
    assert not np.array_equal(want, src)


@pytest.mark.parametrize("a", [0, 1, 128, 255, 256])
def test_match_strengths(a):
    _check_match(R.source(67, 131, seed=11), R.histogram(R.reference()), a)


def test_match_from_device_histograms():
    """The histograms rtsds_hist_u8 leaves on the device, no host round trip."""
    src, ref = R.source(), R.reference()
    x = _dev(src)
    got = T.histogram_match(x, T.image_histogram(x), T.image_histogram(_dev(ref)))
    want, _ = R.match(src, R.histogram(src), R.histogram(ref), 256)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_match_reference_with_empty_bins_at_both_ends():
    _check_match(R.noise(40, 50, seed=12), R.histogram(R.midband(37, 53)), 256)


def test_match_constant_source():
    _check_match(R.constant(20, 31), R.histogram(R.reference()), 256)


def test_match_constant_reference():
    _check_match(R.source(), R.histogram(R.constant(9, 11)), 256)


def test_match_all_zero_reference_is_the_identity():
    src = R.source()
    want = _check_match(src, np.zeros((3, 256), dtype=np.uint32), 256)
    assert np.array_equal(want, src)


def test_match_in_place():
    _check_match(R.source(67, 131, seed=13), R.histogram(R.reference()), 200, in_place=True)


@pytest.mark.parametrize("in_place", [False, True])
def test_match_unaligned_base(in_place):
    src = R.source(67, 131, seed=14)
    _check_match(src, R.histogram(R.reference()), 256, dev_src=_offset_by_one(src), in_place=in_place)


def test_match_into_an_unaligned_destination():
    src = R.source(33, 47, seed=15)
    hs, hr = R.histogram(src), R.histogram(R.reference())
    out = _offset_by_one(np.zeros_like(src))
    got = T.histogram_match(_dev(src), _hist_dev(hs), _hist_dev(hr), out=out)
    assert got is out and torch.equal(got.cpu(), torch.from_numpy(R.match(src, hs, hr, 256)[0]))


def test_match_gta5_size():
    src, hs = _gta5()
    hr = R.histogram(R.reference())
    want, want_lut = R.match(src, hs, hr, 256)
    lut = torch.empty((3, 256), dtype=torch.uint8, device=DEV)
    got = T.histogram_match(_dev(src), _hist_dev(hs), _hist_dev(hr), lut=lut)
    assert torch.equal(lut.cpu(), torch.from_numpy(want_lut))
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# ------------------------------------------------------------------ refusals
def test_python_layer_refuses_wrong_dtype_layout_and_device():
    img = _dev(R.source(8, 12))
    h = T.image_histogram(img)
    for bad in (img.float(), img.permute(2, 0, 1).contiguous(), img[:, ::2], img[..., :2], img.cpu(), img[0]):
        with pytest.raises(RuntimeError):
            T.image_histogram(bad)
        with pytest.raises(RuntimeError):
            T.histogram_match(bad, h, h)
    for bad_h in (h.view(torch.int32).long(), h[:2], h.cpu(), h.view(torch.int32).float(),
                  torch.empty((3, 512), dtype=T._U32, device=DEV)[:, ::2]):
        with pytest.raises(RuntimeError):
            T.histogram_match(img, bad_h, h)
        with pytest.raises(RuntimeError):
            T.histogram_match(img, h, bad_h)
        with pytest.raises(RuntimeError):
            T.image_histogram(img, out=bad_h)
    with pytest.raises(RuntimeError):
        T.histogram_match(img, h, h, out=_dev(R.source(8, 13)))
    with pytest.raises(RuntimeError):
        T.histogram_match(img, h, h, lut=torch.empty((3, 256), dtype=torch.int8, device=DEV))
    with pytest.raises(RuntimeError):
        T.histogram_match(img, h, h, strength=1.5)


# ------------------------------------------------------------------ bank
def test_bank_slots_wrap_around_and_len():
    imgs = [R.noise(9, 14, seed=20), R.sky(12, 7, seed=21), R.source(5, 33, seed=22)]
    bank = T.HistogramBank(2, DEV)
    assert len(bank) == 0 and tuple(bank.data.shape) == (2, 3, 256) and bank.data.dtype == T._U32
    with pytest.raises(IndexError):
        bank.hist(0)
    bank.add([_dev(imgs[0])])
    assert len(bank) == 1 and _same_hist(bank.hist(0), R.histogram(imgs[0]))
    with pytest.raises(IndexError):
        bank.hist(1)
    bank.add([_dev(imgs[1]), _dev(imgs[2])])  # full, then the oldest slot is overwritten
    assert len(bank) == 2
    assert _same_hist(bank.hist(0), R.histogram(imgs[2])) and _same_hist(bank.hist(1), R.histogram(imgs[1]))
    assert bank.hist(1).data_ptr() == bank.data[1].data_ptr()  # written straight into the bank's storage


# ------------------------------------------------------------------ pipeline
SIZE = (32, 48)
REFS = [R.reference(), R.midband(20, 30), R.sky(16, 16)]


def _bank():
    bank = T.HistogramBank(4, DEV)
    bank.add([_dev(r) for r in REFS])
    return bank


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pipeline_end_to_end(dtype):
    """The matched image goes through the existing blur / flip / resize kernels: matching on the
    CPU with the recorded (k, A) and running the pipeline without the transform under the same
    seed gives the same bits."""
    src = R.source()
    blur, flip = T.GaussianBlur((5, 9), (0.1, 5.0)), T.RandomHorizontalFlip(0.5)
    hm = T.HistogramMatching(_bank(), p=1.0, strength=(0.5, 1.0))
    with_t = T.ImagePipeline(SIZE, augment=T.RandomApply([blur, flip, hm], p=1.0))
    without = T.ImagePipeline(SIZE, augment=T.RandomApply([blur, flip], p=1.0))
    img = _dev(src)
    torch.manual_seed(5)
    got = with_t([img], dtype=dtype)
    state = torch.get_rng_state()
    assert torch.equal(img.cpu(), torch.from_numpy(src))  # the caller's image is unchanged
    # the draws, replayed by hand
    torch.manual_seed(5)
    torch.rand(1)
    torch.empty(1).uniform_(0.1, 5.0)
    torch.rand(1)
    assert bool(torch.rand(1) < 1.0)
    k = int(torch.randint(0, 3, (1,)))
    a = R.strength_q8(float(torch.empty(1).uniform_(0.5, 1.0)))
    assert torch.equal(state, torch.get_rng_state())
    assert with_t.last_style == [(k, a)] and 128 <= a <= 256
    matched, _ = R.match(src, R.histogram(src), R.histogram(REFS[k]), a)
    assert not np.array_equal(matched, src)
    torch.manual_seed(5)
    want = without([_dev(matched)], dtype=dtype)
    assert without.last_style == [None]
    assert got.dtype == dtype and torch.equal(got, want)
    torch.manual_seed(5)
    assert not torch.equal(got, without([img], dtype=dtype))  # and the matching did change the batch


def test_pipeline_records_a_style_per_sample():
    hm = T.HistogramMatching(_bank(), p=0.5)
    pipe = T.ImagePipeline(SIZE, augment=T.RandomApply([hm], p=1.0))
    imgs = [_dev(R.source(20 + i, 30, seed=30 + i)) for i in range(6)]
    torch.manual_seed(1)
    got = pipe(imgs, dtype=torch.float32)
    torch.manual_seed(1)
    want_styles = []
    for _ in imgs:
        torch.rand(1)
        if bool(torch.rand(1) < 0.5):
            k = int(torch.randint(0, 3, (1,)))
            want_styles.append((k, R.strength_q8(float(torch.empty(1).uniform_(1.0, 1.0)))))
        else:
            want_styles.append(None)
    assert pipe.last_style == want_styles
    assert any(s is None for s in want_styles) and any(s is not None for s in want_styles)
    plain = T.ImagePipeline(SIZE)
    for n, (img, style) in enumerate(zip(imgs, want_styles)):
        a = img.cpu().numpy()
        if style is not None:
            a, _ = R.match(a, R.histogram(a), R.histogram(REFS[style[0]]), style[1])
        assert torch.equal(got[n], plain([_dev(a)], dtype=torch.float32)[0])


@pytest.mark.parametrize("first", [True, False])
def test_pipeline_with_p_zero_equals_the_pipeline_without(first):
    """Apart from the one coin the transform draws at its position."""
    blur, flip = T.GaussianBlur((5, 9), (0.1, 5.0)), T.RandomHorizontalFlip(0.5)
    hm = T.HistogramMatching(_bank(), p=0.0)
    pipe = T.ImagePipeline(SIZE, augment=T.RandomApply([hm, blur, flip] if first else [blur, flip, hm], p=1.0))
    img = _dev(R.source())
    torch.manual_seed(9)
    got = pipe([img], dtype=torch.float32)
    state = torch.get_rng_state()
    assert pipe.last_style == [None]
    # replay with that coin consumed, then the same blur and flip without any draw left open
    torch.manual_seed(9)
    torch.rand(1)
    if first:
        torch.rand(1)
    sigma = float(torch.empty(1).uniform_(0.1, 5.0))
    flipped = bool(torch.rand(1) < 0.5)
    if not first:
        torch.rand(1)
    assert torch.equal(state, torch.get_rng_state())
    fixed = T.ImagePipeline(SIZE, augment=T.RandomApply([T.GaussianBlur((5, 9), (sigma, sigma)),
                                                         T.RandomHorizontalFlip(1.0 if flipped else 0.0)], p=1.0))
    assert torch.equal(got, fixed([img], dtype=torch.float32))


# ------------------------------------------------------------------ wiring
def test_build_histogram_bank_from_a_cityscapes_tree(tmp_path):
    from PIL import Image

    from rtsds_amd.datasets import CityScapes
    from rtsds_amd.main import build_histogram_bank
    rng = np.random.default_rng(40)
    (tmp_path / "img" / "city").mkdir(parents=True)
    (tmp_path / "gt" / "city").mkdir(parents=True)
    for i in range(5):
        a = (255 * rng.random((16, 32, 3)) ** (0.5 + i)).astype(np.uint8)
        Image.fromarray(a).save(tmp_path / "img" / "city" / f"city_{i:06d}_000019_leftImg8bit.png")
        Image.fromarray(rng.integers(0, 19, (16, 32), dtype=np.uint8)).save(
            tmp_path / "gt" / "city" / f"city_{i:06d}_000019_gtFine_labelTrainIds.png")
    ds = CityScapes(str(tmp_path / "gt"), str(tmp_path / "img"))
    assert len(ds) == 5
    bank = build_histogram_bank(ds, 3, DEV)
    idx = T.bank_indices(5, 3)
    assert idx == [0, 1, 3] and len(bank) == 3
    for slot, i in enumerate(idx):
        assert _same_hist(bank.hist(slot), R.histogram(ds[i][0].numpy()))
    assert len(build_histogram_bank(ds, 64, DEV)) == 5  # a bank larger than the set holds the whole set
