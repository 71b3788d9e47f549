"""Paired random scale-crop on the GPU: rtsds_crop_resize_aa against rtsds_resize_aa on a
contiguous copy of the window (bit-identical) and against the reference arithmetic on the CPU
(oracle/transforms.py), rtsds_crop_resize_nearest against F.interpolate(mode="nearest"), and
the pairing of image and label through ImagePipeline / LabelPipeline / DeviceLoader.

Tolerances: windowed vs copy -- torch.equal; fp32 images vs the CPU -- |err| <= 2e-5 x max|ref|
(the bound tests/test_transforms_gpu.py states for this arithmetic); labels -- torch.equal.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from rtsds_amd import transforms as T  # noqa: E402
from rtsds_amd._lib import lib  # noqa: E402
from rtsds_amd.runtime import stream  # noqa: E402

from tests import cropaug_ref as R  # noqa: E402

DEV = "cuda"
MEAN, STD = T.IMAGENET_MEAN, T.IMAGENET_STD
KIND_DTYPE = {0: torch.float32, 1: torch.bfloat16, 2: torch.int64}


def _case_id(case):
    return "{}x{}-{}-{}x{}".format(*case[0], "_".join(map(str, case[1])), *case[2])


def _img(h, w, c, seed, dtype=torch.uint8):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (h, w, c), generator=g, dtype=torch.uint8)
    if dtype == torch.float32:  # off the integers, as a blurred image is
        x = x.float() + torch.rand((h, w, c), generator=g) - 0.5
    return x


def _ms(c):
    return (torch.tensor(MEAN[:c], dtype=torch.float32, device=DEV),
            torch.tensor(STD[:c], dtype=torch.float32, device=DEV))


def _resize(src, window, kind, size, flip, norm, windowed):
    """src [H, W, C] on the device; the windowed entry, or the plain one on a copy of the window."""
    h, w, c = src.shape
    y0, x0, hc, wc = window
    ho, wo = size
    dst = torch.full((ho, wo, c), -7, dtype=KIND_DTYPE[kind], device=DEV)
    n = lib.rtsds_resize_aa_workspace(c, hc, wc, ho, wo)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    mean, std = _ms(c) if norm else (None, None)
    mp, sp = (mean.data_ptr(), std.data_ptr()) if norm else (None, None)
    u8 = int(src.dtype == torch.uint8)
    clamp = (0, 200) if kind == 2 else (0, -1)
    if windowed:
        lib.rtsds_crop_resize_aa(src.data_ptr(), u8, c, h, w, y0, x0, hc, wc, dst.data_ptr(), kind, ho, wo, flip, mp,
                                 sp, *clamp, ws.data_ptr(), n, stream())
    else:
        copy = src[y0:y0 + hc, x0:x0 + wc].contiguous()
        lib.rtsds_resize_aa(copy.data_ptr(), u8, c, hc, wc, dst.data_ptr(), kind, ho, wo, flip, mp, sp, *clamp,
                            ws.data_ptr(), n, stream())
    torch.cuda.synchronize()
    return dst


@pytest.mark.parametrize("case", R.AA_CASES, ids=_case_id)
@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_windowed_is_bit_identical_to_the_copy(case, c, dtype):
    (h, w), window, size = case
    src = _img(h, w, c, seed=h + w + c, dtype=dtype).to(DEV)
    for kind in (0, 1, 2):
        for norm in ((False, True) if kind != 2 else (False,)):
            for flip in (0, 1):
                got = _resize(src, window, kind, size, flip, norm, windowed=True)
                want = _resize(src, window, kind, size, flip, norm, windowed=False)
                assert torch.equal(got, want), (kind, norm, flip)


@pytest.mark.parametrize("case", R.AA_CASES + [R.GTA_CASE], ids=_case_id)
@pytest.mark.parametrize("flip", [0, 1])
def test_windowed_against_the_reference_arithmetic(case, flip):
    (h, w), window, size = case
    img = _img(h, w, 3, seed=h + flip, dtype=torch.float32)
    ref = R.image_ref(img, window, size, flip, MEAN, STD)
    got = _resize(img.to(DEV), window, 0, size, flip, True, windowed=True).permute(2, 0, 1).cpu()
    err = (got - ref).abs().max().item()
    print(f"{case} flip {flip}: err {err:.3e}, bound {2e-5 * ref.abs().max().item():.3e}")
    assert err <= 2e-5 * ref.abs().max().item(), err


def _label(h, w, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, 19, (h, w), generator=g, dtype=torch.uint8)
    lab[torch.rand((h, w), generator=g) < 0.2] = 255
    return lab.to(dtype)


@pytest.mark.parametrize("win,size", R.NEAREST_CASES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_nearest_label_window(win, size, dtype):
    hc, wc = win
    h, w = hc + 5, wc + 9
    lab = _label(h, w, seed=hc + wc, dtype=dtype)
    dev = lab.to(DEV)
    ho, wo = size
    for y0, x0 in ((0, 0), (h - hc, w - wc)):        # both corners
        for flip in (0, 1):
            for clamp in (None, (0, 19)):
                out = torch.full((ho, wo), -7, dtype=torch.int64, device=DEV)
                lo, hi = clamp or (0, -1)
                lib.rtsds_crop_resize_nearest(dev.data_ptr(), int(dtype == torch.int64), h, w, y0, x0, hc, wc,
                                              out.data_ptr(), ho, wo, flip, lo, hi, stream())
                torch.cuda.synchronize()
                want = R.nearest_label(lab, (y0, x0, hc, wc), size, flip, clamp)
                assert torch.equal(out.cpu(), want), (y0, x0, flip, clamp)


# ------------------------------------------------------------------ pipelines
SIZE = (32, 48)


def _sample(seed=31):
    return _img(64, 96, 3, seed), _label(64, 96, seed + 1, torch.uint8)


def _pipes(labels, p=1.0):
    aug = T.RandomApply([T.RandomResizedCrop(scale=(0.25, 1.0), ratio=(1.0, 2.0)),
                         T.RandomHorizontalFlip(1.0, labels=labels)], p=p)
    return T.ImagePipeline(SIZE, augment=aug), T.LabelPipeline(SIZE, clamp=(0, 19))


def _redraw(seed):
    torch.manual_seed(seed)
    torch.rand(1)                                                     # RandomApply's coin
    window = R.get_params(64, 96, (0.25, 1.0), (1.0, 2.0))
    torch.rand(1)                                                     # the flip's coin
    return window


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("paired", [True, False])
def test_pipeline_pairs_image_and_label(seed, paired):
    img, lab = _sample()
    ip, lp = _pipes(labels=paired)
    torch.manual_seed(seed)
    x = ip([img.to(DEV)], dtype=torch.float32)
    y = lp([lab.to(DEV)], ip.last_geometry)
    torch.cuda.synchronize()
    window = _redraw(seed)
    assert ip.last_geometry == [window + (paired,)] and ip.last_geometry[0].source == (64, 96)
    ref = R.image_ref(img, window, SIZE, True, MEAN, STD)
    assert (x[0].cpu() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
    assert x.is_contiguous(memory_format=torch.channels_last)
    assert y.shape == (1, 1) + SIZE and y.dtype == torch.int64
    assert torch.equal(y[0, 0].cpu(), R.nearest_label(lab, window, SIZE, flip=paired, clamp=(0, 19)))
    # int64 labels (decoded GTA5 ids) take the same path, with no float copy
    y64 = lp([lab.long().to(DEV)], ip.last_geometry)
    assert torch.equal(y64, y)


def test_paired_flip_without_a_window_mirrors_the_antialiased_label():
    img, lab = _sample()
    ip = T.ImagePipeline(SIZE, augment=T.RandomApply([T.RandomHorizontalFlip(1.0, labels=True)], p=1.0))
    lp = T.LabelPipeline(SIZE, clamp=(0, 19))
    ip([img.to(DEV)], dtype=torch.float32)
    assert ip.last_geometry == [(0, 0, 64, 96, True)]
    got = lp([lab.to(DEV)], ip.last_geometry)
    want = lp([lab.flip(-1).contiguous().to(DEV)])
    assert torch.equal(got, want)
    assert not torch.equal(got, lp([lab.to(DEV)]))


def test_failed_coin_leaves_both_pipelines_as_they_were():
    img, lab = _sample()
    ip, lp = _pipes(labels=True, p=0.0)
    x = ip([img.to(DEV), img.to(DEV)], dtype=torch.float32)
    assert ip.last_geometry == [None, None]
    y = lp([lab.to(DEV), lab.to(DEV)], ip.last_geometry)
    plain = T.ImagePipeline(SIZE)
    assert torch.equal(x, plain([img.to(DEV), img.to(DEV)], dtype=torch.float32))
    assert plain.last_geometry == [None, None]
    assert torch.equal(y, lp([lab.to(DEV), lab.to(DEV)]))


def test_device_loader_over_raw_samples_of_different_sizes():
    sizes = [(64, 96), (50, 70), (37, 53), (80, 64)]
    raw = [(_img(h, w, 3, seed=h), _label(h, w, seed=w, dtype=torch.uint8)) for h, w in sizes]
    batches = [T.collate_raw(raw[:2]), T.collate_raw(raw[2:])]
    ip, lp = _pipes(labels=True)
    import rtsds_amd
    torch.manual_seed(4)
    with rtsds_amd.precision(torch.float32):
        out = list(T.DeviceLoader(batches, ip, lp))
    torch.manual_seed(4)
    assert len(out) == 2
    for b, (x, y) in enumerate(out):
        assert x.shape == (2, 3) + SIZE and x.dtype == torch.float32 and x.device.type == "cuda"
        assert x.is_contiguous(memory_format=torch.channels_last)
        assert y.shape == (2, 1) + SIZE and y.dtype == torch.int64
        for n in range(2):
            img, lab = raw[2 * b + n]
            h, w = sizes[2 * b + n]
            torch.rand(1)
            window = R.get_params(h, w, (0.25, 1.0), (1.0, 2.0))
            torch.rand(1)
            ref = R.image_ref(img, window, SIZE, True, MEAN, STD)
            # slot n of the NHWC batch holds this sample's HWC image
            slot = x[n].permute(1, 2, 0)
            assert slot.is_contiguous()
            assert (slot.permute(2, 0, 1).cpu() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
            assert torch.equal(y[n, 0].cpu(), R.nearest_label(lab, window, SIZE, flip=True, clamp=(0, 19)))
