"""Device-side input pipeline: the reference's torchvision transforms (main.py:25-108) as HIP
kernels (csrc/data.hip) over decoded uint8 HWC images in HBM.

Reference pipelines (main.py:60-96), reproduced here per sample of a batch:

* Cityscapes image:  Resize(image_size, antialias=True) -> Normalize(mean, std)
* Cityscapes label:  Resize(image_size, antialias=True) -> IntRangeTransformer(0, num_classes)
* GTA5 image:        [RandomApply([GaussianBlur(k, sigma), RandomHorizontalFlip(p),
                     ColorJitter(b, c, s, h)], p)] -> Resize(image_size) -> Normalize(mean, std);
                     blur and jitter run in the order the config lists them (they do not
                     commute, because of the clamps); the flip commutes with both and stays
                     fused into the resize
* GTA5 label:        Resize(image_size)   (the augmentation flips the image only, as the
                     reference's pipeline does)

Beyond the reference, opt-in: RandomResizedCrop in the augmentation list draws a window of the
source image per sample; the image's resize reads that window in place (rtsds_crop_resize_aa)
and the label takes the same window through a nearest resample (rtsds_crop_resize_nearest).
RandomHorizontalFlip(labels=True) mirrors the label with the image.  ImagePipeline records what
it did per sample in ``last_geometry``; DeviceLoader hands that to the LabelPipeline.
HistogramMatching matches each channel's histogram of the decoded uint8 image to that of a target
image drawn from a HistogramBank (csrc/histmatch.hip: rtsds_hist_u8, rtsds_hist_match), ahead of
the blur and the jitter; ``last_style`` records the draw per sample.
FourierAdaptation (FDA, Yang & Soatto 2020) replaces the low-frequency amplitudes of the decoded
image's spectrum by those of a target image drawn from a SpectrumBank (csrc/fda.hip:
rtsds_fda_spectrum, rtsds_fda_apply), in uint8, after the histogram matching and ahead of the
blur and the jitter; ``last_spectral`` records the draw per sample.

The image comes out in the network's input layout (NHWC, the runtime compute dtype), so the
model's input packing is a no-op; labels come out int64 [N, 1, H, W] as the reference's loaders
deliver them (train.py squeezes dim 1).  Random decisions draw from torch's CPU generator in
torchvision's call order (RandomApply's coin, then per listed transform: GaussianBlur's sigma,
the flip coin, ColorJitter's permutation and factors, RandomResizedCrop's get_params,
HistogramMatching's and FourierAdaptation's coin and -- if taken -- bank entry and strength).
"""
import ctypes
import math

import torch

from ._lib import lib
from .functional import _U32
from .runtime import CL, compute_dtype, require_hip, stream, workspace

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _check(code, what):
    if code != 0:
        raise RuntimeError(f"rtsds_amd.transforms: {what} failed (status {code})")


class GaussianBlur:
    """torchvision GaussianBlur(kernel_size, sigma): sigma ~ U(sigma_min, sigma_max) per call."""

    def __init__(self, kernel_size, sigma=(0.1, 2.0)):
        ks = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        if any(k <= 0 or k % 2 == 0 for k in ks):
            raise ValueError("Kernel size value should be an odd and positive number.")
        self.kernel_size = ks
        self.sigma = (sigma, sigma) if isinstance(sigma, (int, float)) else tuple(sigma)

    def params(self):
        return float(torch.empty(1).uniform_(self.sigma[0], self.sigma[1]).item())


class RandomHorizontalFlip:
    """RandomHorizontalFlip(p).  The reference's pipeline mirrors the image only (main.py:86-96);
    ``labels=True`` mirrors the label with it."""

    def __init__(self, p=0.5, labels=False):
        self.p = p
        self.labels = bool(labels)


def _ascending_pair(name, value):
    ok = isinstance(value, (tuple, list)) and len(value) == 2 and \
        all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in value)
    if not ok or not 0 < value[0] <= value[1] or not math.isfinite(value[1]):
        raise ValueError(f"{name} should be a pair of positive numbers (min, max).")
    return float(value[0]), float(value[1])


class RandomResizedCrop:
    """torchvision RandomResizedCrop's window: a share ``scale`` of the area at an aspect ratio
    (w / h) from ``ratio``, log-uniform.  The output size is the pipeline's: the window goes to
    the resize."""

    def __init__(self, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
        self.scale = _ascending_pair("scale", scale)
        self.ratio = _ascending_pair("ratio", ratio)

    def params(self, h, w):
        """(y0, x0, hc, wc) in get_params' draw order: up to 10 tries of (area, log ratio) and,
        for the first that fits, the two origins; else the ratio-clamped centre crop."""
        area = h * w
        log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        for _ in range(10):
            ta = area * torch.empty(1).uniform_(self.scale[0], self.scale[1]).item()
            ar = math.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1]).item())
            wc = int(round(math.sqrt(ta * ar)))
            hc = int(round(math.sqrt(ta / ar)))
            if 0 < wc <= w and 0 < hc <= h:
                y0 = int(torch.randint(0, h - hc + 1, size=(1,)).item())
                x0 = int(torch.randint(0, w - wc + 1, size=(1,)).item())
                return y0, x0, hc, wc
        in_ratio = float(w) / float(h)
        if in_ratio < self.ratio[0]:
            wc = w
            hc = int(round(wc / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            hc = h
            wc = int(round(hc * self.ratio[1]))
        else:
            wc, hc = w, h
        return (h - hc) // 2, (w - wc) // 2, hc, wc


def _jitter_range(name, value, center, lo_bound, hi_bound):
    """torchvision ColorJitter._check_input: a number x means [center - x, center + x] (floored
    at 0 around center 1), a pair is taken as given; None when the range is the identity."""
    if isinstance(value, bool):
        raise ValueError(f"{name} should be a single number or a sequence of two numbers.")
    if isinstance(value, (int, float)):
        if value < 0:
            raise ValueError(f"If {name} is a single number, it must be non negative.")
        rng = [center - float(value), center + float(value)]
        if center == 1:
            rng[0] = max(rng[0], 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2 and \
            all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in value):
        rng = [float(value[0]), float(value[1])]
    else:
        raise ValueError(f"{name} should be a single number or a sequence of two numbers.")
    if not lo_bound <= rng[0] <= rng[1] <= hi_bound:
        raise ValueError(f"{name} values should be ordered and between {lo_bound} and {hi_bound}, got {rng}.")
    return None if rng[0] == rng[1] == center else (rng[0], rng[1])


class ColorJitter:
    """torchvision ColorJitter(brightness, contrast, saturation, hue): per call a permutation of
    the four adjustments and one factor for each that is on.  ``value_range`` is the image's
    scale (the clamp bound): 255 for the decoded images of this pipeline, 1 for torchvision's
    float convention."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, value_range=255.0):
        inf = float("inf")
        self.brightness = _jitter_range("brightness", brightness, 1, 0.0, inf)
        self.contrast = _jitter_range("contrast", contrast, 1, 0.0, inf)
        self.saturation = _jitter_range("saturation", saturation, 1, 0.0, inf)
        self.hue = _jitter_range("hue", hue, 0, -0.5, 0.5)
        if not value_range > 0:
            raise ValueError("value_range should be positive.")
        self.value_range = float(value_range)

    def params(self):
        """(order, fb, fc, fs, fh) in get_params' draw order; None for an op that is off."""
        order = tuple(int(i) for i in torch.randperm(4))
        fs = tuple(None if r is None else float(torch.empty(1).uniform_(r[0], r[1]))
                   for r in (self.brightness, self.contrast, self.saturation, self.hue))
        return (order,) + fs


class HistogramMatching:
    """Per-channel histogram matching of the decoded image to a target image drawn from ``bank``
    (anything with ``len()`` and ``hist(k)``: HistogramBank), with probability ``p`` and a blend
    strength ~ U(strength) in [0, 1] (1 = full matching).  Not in the reference."""

    def __init__(self, bank, p=0.5, strength=(1.0, 1.0)):
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
            raise ValueError("p should be a number in [0, 1].")
        if isinstance(strength, (int, float)) and not isinstance(strength, bool):
            strength = (strength, strength)
        ok = isinstance(strength, (tuple, list)) and len(strength) == 2 and \
            all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in strength)
        if not ok or not 0.0 <= strength[0] <= strength[1] <= 1.0:
            raise ValueError("strength should be a pair of numbers ordered within [0, 1].")
        self.bank = bank
        self.p = float(p)
        self.strength = (float(strength[0]), float(strength[1]))

    def params(self):
        """None, or (k, A): the bank entry and the strength in Q8.  Draws: the coin, then -- only
        if it is taken -- the entry and the strength."""
        if not bool(torch.rand(1) < self.p):
            return None
        n = len(self.bank)
        if n == 0:
            raise RuntimeError("rtsds_amd.transforms: HistogramMatching drew from an empty bank")
        k = int(torch.randint(0, n, (1,)).item())
        s = float(torch.empty(1).uniform_(self.strength[0], self.strength[1]).item())
        return k, _strength_q8(s)


FDA_MAX_BAND = 64  # rtsds_fda_*: 1 <= b <= 64, 2b + 1 <= min(h, w), h * w <= 2^24
FDA_MAX_PIXELS = 1 << 24


def _check_band(h, w, b):
    if not 1 <= b <= FDA_MAX_BAND or 2 * b + 1 > min(h, w) or h * w > FDA_MAX_PIXELS:
        raise ValueError(f"rtsds_amd.transforms: a Fourier band of b = {b} on a {h} x {w} image is outside the kernels' "
                         f"limits (1 <= b <= {FDA_MAX_BAND}, 2b + 1 <= min(h, w), h * w <= 2^24)")


class FourierAdaptation:
    """Fourier Domain Adaptation (Yang & Soatto, CVPR 2020): with probability ``p`` the amplitudes
    of the (2b+1) x (2b+1) lowest frequencies of the decoded image, b = max(1, floor(min(h, w) *
    beta)), are blended by a strength ~ U(strength) in [0, 1] (1 = replaced) towards those of a
    target image drawn from ``bank`` (anything with ``len()``, ``b`` and ``amp(k)``: SpectrumBank);
    the phase is kept.  Not in the reference."""

    def __init__(self, bank, p=0.5, beta=0.01, strength=(1.0, 1.0)):
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
            raise ValueError("p should be a number in [0, 1].")
        if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0.0 < beta < 0.5:
            raise ValueError("beta should be a number in (0, 0.5).")
        if isinstance(strength, (int, float)) and not isinstance(strength, bool):
            strength = (strength, strength)
        ok = isinstance(strength, (tuple, list)) and len(strength) == 2 and \
            all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in strength)
        if not ok or not 0.0 <= strength[0] <= strength[1] <= 1.0:
            raise ValueError("strength should be a pair of numbers ordered within [0, 1].")
        self.bank = bank
        self.p = float(p)
        self.beta = float(beta)
        self.strength = (float(strength[0]), float(strength[1]))

    def band(self, h, w):
        """b for an h x w image; raises where the kernels' limits are broken or the bank was built
        for another band."""
        b = max(1, int(math.floor(min(h, w) * self.beta)))
        _check_band(h, w, b)
        have = getattr(self.bank, "b", None)
        if have is not None and have != b:
            raise ValueError(f"rtsds_amd.transforms: FourierAdaptation(beta={self.beta}) needs a band of b = {b} on a "
                             f"{h} x {w} image, the bank holds b = {have}")
        return b

    def params(self):
        """None, or (k, strength): the bank entry and the blend.  Draws: the coin, then -- only if
        it is taken -- the entry and the strength (HistogramMatching's order)."""
        if not bool(torch.rand(1) < self.p):
            return None
        n = len(self.bank)
        if n == 0:
            raise RuntimeError("rtsds_amd.transforms: FourierAdaptation drew from an empty bank")
        k = int(torch.randint(0, n, (1,)).item())
        s = float(torch.empty(1).uniform_(self.strength[0], self.strength[1]).item())
        return k, s


class RandomApply:
    """RandomApply(transforms, p): the listed transforms all run with probability p."""

    def __init__(self, transforms, p=0.5):
        self.transforms = list(transforms)
        self.p = p


def augmentation_loader(config, probability, bank=None, *, spectrum_bank=None):
    """main.py:46-58 / 25-44: RandomApply over the configured augmentations.  ``bank``: the
    target histograms the key HistogramMatching draws from (main.build_histogram_bank);
    ``spectrum_bank``: the target amplitudes of the key FourierAdaptation
    (main.build_spectrum_bank)."""
    aug = config.augmentation
    out = []
    for key in aug.keys():
        if key == "GaussianBlur":
            c = aug["GaussianBlur"]
            out.append(GaussianBlur(kernel_size=[int(i) for i in str(c["kernel_size"]).split(",")],
                                    sigma=[float(i) for i in str(c["sigma"]).split(",")]))
        elif key == "RandomHorizontalFlip":
            c = aug["RandomHorizontalFlip"]
            out.append(RandomHorizontalFlip(p=c["p"], labels=c.get("labels", False)))
        elif key == "RandomResizedCrop":
            c = aug["RandomResizedCrop"] or {}
            out.append(RandomResizedCrop(**{k: [float(i) for i in str(c[k]).split(",")]
                                            for k in ("scale", "ratio") if k in c}))
        elif key == "ColorJitter":
            c = aug["ColorJitter"]
            out.append(ColorJitter(brightness=c["brightness"], contrast=c["contrast"], saturation=c["saturation"],
                                   hue=c["hue"]))
        elif key == "HistogramMatching":
            c = aug["HistogramMatching"]
            if bank is None:
                raise RuntimeError("rtsds_amd.transforms: the augmentation HistogramMatching needs a bank of "
                                   "target histograms (augmentation_loader(config, p, bank=...))")
            strength = [float(i) for i in str(c["strength"]).split(",")] if "strength" in c else [1.0, 1.0]
            out.append(HistogramMatching(bank, p=c["p"], strength=strength * 2 if len(strength) == 1 else strength))
        elif key == "FourierAdaptation":
            c = aug["FourierAdaptation"] or {}
            if spectrum_bank is None:
                raise RuntimeError("rtsds_amd.transforms: the augmentation FourierAdaptation needs a bank of target "
                                   "amplitudes (augmentation_loader(config, p, spectrum_bank=...))")
            strength = [float(i) for i in str(c["strength"]).split(",")] if "strength" in c else [1.0, 1.0]
            out.append(FourierAdaptation(spectrum_bank, p=c.get("p", 0.5), beta=c.get("beta", 0.01),
                                         strength=strength * 2 if len(strength) == 1 else strength))
        elif key == "ColorJitterWithRandomBrightness":
            raise NotImplementedError("rtsds_amd.transforms: ColorJitterWithRandomBrightness is not implemented "
                                      "(the reference config has it commented out, config.yaml:118-123)")
    return RandomApply(out, p=probability)


def _sample_draws(augment, h=None, w=None):
    """([(transform, its draw)] for the blur / jitter in list order, flip, window, flip_label)
    for one sample of source size (h, w), drawing in torchvision's order.  window is
    RandomResizedCrop's (y0, x0, hc, wc) or None; flip_label says the flip came from a
    RandomHorizontalFlip(labels=True).  Geometry takes effect at the resize wherever its key
    stands (the window is uniform in x, so a flip ahead of it changes no distribution)."""
    return _sample_draws_styled(augment, h, w)[:4]


def _sample_draws_styled(augment, h=None, w=None):
    """_sample_draws' four and, fifth, HistogramMatching's draw (None, or (its bank, k, A)), taken
    at the transform's position in the list; the matching itself acts on the decoded image,
    ahead of the blur and the jitter, wherever its key stands."""
    return _sample_draws_all(augment, h, w)[:5]


def _sample_draws_all(augment, h=None, w=None):
    """_sample_draws_styled's five and, sixth, FourierAdaptation's draw (None, or (its bank, k,
    strength)), taken at the transform's position in the list like the others; a list without
    the transform draws nothing for it."""
    if augment is None or not augment.transforms:
        return [], False, None, False, None, None
    if augment.p < torch.rand(1):
        return [], False, None, False, None, None
    ops, flip, window, flip_label, style, spectral = [], False, None, False, None, None
    for t in augment.transforms:
        if isinstance(t, (GaussianBlur, ColorJitter)):
            ops.append((t, t.params()))
        elif isinstance(t, RandomHorizontalFlip):
            flip = bool(torch.rand(1) < t.p)
            flip_label = flip and t.labels
        elif isinstance(t, RandomResizedCrop):
            if h is None or w is None:
                raise RuntimeError("rtsds_amd.transforms: RandomResizedCrop draws for a source size")
            window = t.params(h, w)
        elif isinstance(t, HistogramMatching):
            drawn = t.params()
            style = None if drawn is None else (t.bank,) + drawn
        elif isinstance(t, FourierAdaptation):
            drawn = t.params()
            spectral = None if drawn is None else (t,) + drawn
    return ops, flip, window, flip_label, style, spectral


def _decisions(augment):
    """([(transform, its draw)] for the blur / jitter in list order, flip) for one sample of a
    list without geometry that needs the source size."""
    return _sample_draws(augment)[:2]


class Geometry(tuple):
    """One sample's entry of ImagePipeline.last_geometry: (y0, x0, hc, wc, flip_label), the
    window in the source image (the whole image without a crop) and whether the label is to be
    mirrored; ``source`` is the source image's (h, w), which the label must share."""

    def __new__(cls, y0, x0, hc, wc, flip_label, source):
        self = super().__new__(cls, (int(y0), int(x0), int(hc), int(wc), bool(flip_label)))
        self.source = (int(source[0]), int(source[1]))
        return self


def color_jitter(img, order, fb, fc, fs, fh, value_range=255.0, out=None):
    """ColorJitter's forward with the draws given: the adjustments 0 brightness, 1 contrast,
    2 saturation, 3 hue applied in ``order`` with their factors (None = off) to an HWC RGB
    device image (uint8, or fp32 in [0, value_range]).  fp32 HWC out; ``out`` may be ``img``
    itself when that is fp32."""
    if img.dtype not in (torch.uint8, torch.float32) or img.dim() != 3 or not img.is_contiguous():
        raise RuntimeError("rtsds_amd.transforms: color_jitter takes a contiguous HWC uint8 or fp32 image")
    h, w, c = img.shape
    if out is None:
        out = torch.empty((h, w, c), dtype=torch.float32, device=img.device)
    elif out.dtype != torch.float32 or out.shape != img.shape or not out.is_contiguous() or out.device != img.device:
        raise RuntimeError("rtsds_amd.transforms: color_jitter writes a contiguous fp32 image of the source's shape")
    factors = (fb, fc, fs, fh)
    mask = sum(1 << k for k, f in enumerate(factors) if f is not None)
    fb, fc, fs, fh = (ident if f is None else f for f, ident in zip(factors, (1.0, 1.0, 1.0, 0.0)))
    # contrast: the partial sums of the grey mean
    ws = workspace(lib.rtsds_color_jitter_workspace(h, w), img.device) if mask & 2 else None
    _check(lib.rtsds_color_jitter(img.data_ptr(), int(img.dtype == torch.uint8), out.data_ptr(), c, h, w,
                                  (ctypes.c_int * 4)(*order), mask, fb, fc, fs, fh, value_range,
                                  ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                  stream()), "color jitter")
    return out


def _strength_q8(strength):
    """A = floor(strength * 256 + 0.5): the blend weight of rtsds_hist_match, 0..256."""
    if not 0.0 <= strength <= 1.0:
        raise RuntimeError(f"rtsds_amd.transforms: a matching strength in [0, 1] expected, got {strength}")
    return int(math.floor(strength * 256 + 0.5))


def _check_rgb_u8(img, what):
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or \
            not img.is_contiguous():
        raise RuntimeError(f"rtsds_amd.transforms: {what} takes a contiguous HWC uint8 [H, W, 3] image")
    require_hip(img)


def _check_hist(hist, device, what):
    if not isinstance(hist, torch.Tensor) or hist.dtype != _U32 or tuple(hist.shape) != (3, 256) or \
            not hist.is_contiguous() or hist.device != device:
        raise RuntimeError(f"rtsds_amd.transforms: {what} must be a contiguous {_U32} [3, 256] tensor on the image's "
                           "device")


def image_histogram(img, out=None):
    """The per-channel histogram of a uint8 HWC [H, W, 3] device image: uint32 [3, 256] on its
    device (rtsds_hist_u8; ``out`` is overwritten, not added to)."""
    _check_rgb_u8(img, "image_histogram")
    if out is None:
        out = torch.empty((3, 256), dtype=_U32, device=img.device)
    else:
        _check_hist(out, img.device, "image_histogram: out")
    h, w, c = img.shape
    _check(lib.rtsds_hist_u8(img.data_ptr(), c, h, w, out.data_ptr(), stream()), "image histogram")
    return out


def _hist_match_q8(img, hist_src, hist_ref, a, out=None, lut=None):
    _check_rgb_u8(img, "histogram_match")
    _check_hist(hist_src, img.device, "histogram_match: hist_src")
    _check_hist(hist_ref, img.device, "histogram_match: hist_ref")
    if out is None:
        out = torch.empty_like(img)
    elif out is not img:
        _check_rgb_u8(out, "histogram_match: out")
        if out.shape != img.shape or out.device != img.device:
            raise RuntimeError("rtsds_amd.transforms: histogram_match writes an image of the source's shape and device")
    if lut is not None and (not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or
                            tuple(lut.shape) != (3, 256) or not lut.is_contiguous() or lut.device != img.device):
        raise RuntimeError("rtsds_amd.transforms: histogram_match: lut must be a contiguous uint8 [3, 256] tensor on "
                           "the image's device")
    h, w, c = img.shape
    _check(lib.rtsds_hist_match(img.data_ptr(), out.data_ptr(), c, h, w, hist_src.data_ptr(), hist_ref.data_ptr(),
                                int(a), lut.data_ptr() if lut is not None else None, stream()), "histogram match")
    return out


def histogram_match(img, hist_src, hist_ref, strength=1.0, out=None, lut=None):
    """``img`` (uint8 HWC [H, W, 3], device) with each channel's histogram ``hist_src`` matched to
    ``hist_ref`` (both uint32 [3, 256]: image_histogram of the image and of the reference image),
    blended with the source by ``strength`` in [0, 1] in Q8.  uint8 HWC out; ``out`` may be
    ``img``.  ``lut`` (uint8 [3, 256]) receives the per-channel value map."""
    return _hist_match_q8(img, hist_src, hist_ref, _strength_q8(float(strength)), out, lut)


class HistogramBank:
    """The histograms of up to ``capacity`` target images on the device (uint32
    [capacity, 3, 256], 3 KB each): a ring, the oldest entry is overwritten when full."""

    def __init__(self, capacity, device="cuda"):
        if int(capacity) < 1:
            raise ValueError("capacity should be positive.")
        self.data = torch.zeros((int(capacity), 3, 256), dtype=torch.int32, device=device).view(_U32)
        self._next = 0
        self._filled = 0

    def add(self, images):
        """One histogram per uint8 HWC device image, each written straight into its slot."""
        for img in images:
            image_histogram(img, out=self.data[self._next])
            self._next = (self._next + 1) % self.data.shape[0]
            self._filled = min(self._filled + 1, self.data.shape[0])

    def __len__(self):
        return self._filled

    def hist(self, k):
        if not 0 <= k < self._filled:
            raise IndexError(f"histogram {k} of a bank of {self._filled}")
        return self.data[k]


def _check_band_tensor(t, b, last, device, what):
    shape = (3, 2 * b + 1, b + 1) + last
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or \
            t.device != device:
        raise RuntimeError(f"rtsds_amd.transforms: {what} must be a contiguous fp32 {list(shape)} tensor on the image's "
                           "device")


def _fda_spectrum(img, b, spec, amp):
    h, w, c = img.shape
    ws = workspace(lib.rtsds_fda_workspace(h, w, b), img.device)  # the row-stage partials
    _check(lib.rtsds_fda_spectrum(img.data_ptr(), c, h, w, b, spec.data_ptr() if spec is not None else None,
                                  amp.data_ptr() if amp is not None else None, ws.data_ptr(), ws.numel(), stream()),
           "band spectrum")


def band_spectrum(img, b, spec=None, amp=None):
    """(spec, amp_norm) of a uint8 HWC [H, W, 3] device image: the DFT coefficients F(u, v) of the
    band u = -b..b, v = 0..b as fp32 [3, 2b+1, b+1, 2] (re, im; the other half is the conjugate
    mirror) and |F| / (H W) as fp32 [3, 2b+1, b+1], the size-independent form a SpectrumBank keeps
    (rtsds_fda_spectrum; ``spec`` / ``amp`` are overwritten)."""
    _check_rgb_u8(img, "band_spectrum")
    b = int(b)
    _check_band(img.shape[0], img.shape[1], b)
    if spec is None:
        spec = torch.empty((3, 2 * b + 1, b + 1, 2), dtype=torch.float32, device=img.device)
    else:
        _check_band_tensor(spec, b, (2,), img.device, "band_spectrum: spec")
    if amp is None:
        amp = torch.empty((3, 2 * b + 1, b + 1), dtype=torch.float32, device=img.device)
    else:
        _check_band_tensor(amp, b, (), img.device, "band_spectrum: amp")
    _fda_spectrum(img, b, spec, amp)
    return spec, amp


def fourier_adapt(img, spec_src, amp_ref, strength=1.0, out=None, dtype=torch.uint8):
    """``img`` (uint8 HWC [H, W, 3], device) with the amplitudes of its band ``spec_src``
    (band_spectrum of the image) blended by ``strength`` in [0, 1] towards ``amp_ref`` (the
    normalised amplitudes of a target image of any size), the phase kept (rtsds_fda_apply).  HWC
    out, clamped to [0, 255]: uint8 (rounded half to even; ``out`` may be ``img``) or fp32."""
    _check_rgb_u8(img, "fourier_adapt")
    if dtype not in (torch.uint8, torch.float32):
        raise RuntimeError("rtsds_amd.transforms: fourier_adapt writes uint8 or fp32")
    if not isinstance(spec_src, torch.Tensor) or spec_src.dim() != 4:
        raise RuntimeError("rtsds_amd.transforms: fourier_adapt: spec_src must be the [3, 2b+1, b+1, 2] band of the image")
    b = int(spec_src.shape[2]) - 1
    h, w, c = img.shape
    _check_band(h, w, b)
    _check_band_tensor(spec_src, b, (2,), img.device, "fourier_adapt: spec_src")
    _check_band_tensor(amp_ref, b, (), img.device, "fourier_adapt: amp_ref")
    strength = float(strength)
    if not 0.0 <= strength <= 1.0:
        raise RuntimeError(f"rtsds_amd.transforms: a blend strength in [0, 1] expected, got {strength}")
    if out is None:
        out = torch.empty((h, w, c), dtype=dtype, device=img.device)
    elif out is not img:
        if not isinstance(out, torch.Tensor) or out.dtype != dtype or out.shape != img.shape or not out.is_contiguous() or \
                out.device != img.device:
            raise RuntimeError("rtsds_amd.transforms: fourier_adapt writes a contiguous image of the source's shape and "
                               "device in the dtype asked for")
    elif dtype != torch.uint8:
        raise RuntimeError("rtsds_amd.transforms: fourier_adapt works in place in uint8 only")
    _check(lib.rtsds_fda_apply(img.data_ptr(), out.data_ptr(), int(dtype == torch.uint8), c, h, w, b, spec_src.data_ptr(),
                               amp_ref.data_ptr(), strength, stream()), "fourier adapt")
    return out


class SpectrumBank:
    """The normalised band amplitudes |F| / (h w) of up to ``capacity`` target images on the device
    (fp32 [capacity, 3, 2b+1, b+1]): a ring, the oldest entry is overwritten when full.  The
    images may have any size the band fits in: an entry is in cycles per image."""

    def __init__(self, capacity, b, device="cuda"):
        if int(capacity) < 1:
            raise ValueError("capacity should be positive.")
        if not 1 <= int(b) <= FDA_MAX_BAND:
            raise ValueError(f"b should be in [1, {FDA_MAX_BAND}].")
        self.b = int(b)
        self.data = torch.zeros((int(capacity), 3, 2 * self.b + 1, self.b + 1), dtype=torch.float32, device=device)
        self._next = 0
        self._filled = 0

    def add(self, images):
        """One entry per uint8 HWC device image, each written straight into its slot."""
        for img in images:
            _check_rgb_u8(img, "SpectrumBank.add")
            _check_band(img.shape[0], img.shape[1], self.b)
            _fda_spectrum(img, self.b, None, self.data[self._next])
            self._next = (self._next + 1) % self.data.shape[0]
            self._filled = min(self._filled + 1, self.data.shape[0])

    def __len__(self):
        return self._filled

    def amp(self, k):
        if not 0 <= k < self._filled:
            raise IndexError(f"spectrum {k} of a bank of {self._filled}")
        return self.data[k]


def bank_indices(n, k):
    """The min(n, k) dataset indices floor(i * n / min(n, k)): an even spread over n samples."""
    m = min(int(n), int(k))
    return [i * int(n) // m for i in range(m)] if m > 0 else []


def _as_hwc_u8(img):
    if img.dtype != torch.uint8:
        raise RuntimeError("rtsds_amd.transforms: decoded uint8 images expected")
    if img.dim() == 2:
        img = img.unsqueeze(-1)
    return img.contiguous()


class ImagePipeline:
    """Resize(size, antialias=True) [after the optional augmentation] -> Normalize, into slot n
    of an NHWC batch in the compute dtype."""

    def __init__(self, size, mean=IMAGENET_MEAN, std=IMAGENET_STD, augment=None):
        self.size = (int(size[0]), int(size[1]))
        self.mean, self.std = tuple(mean), tuple(std)
        self.augment = augment
        self.last_geometry = None  # per sample of the last batch: None or a Geometry
        self.last_style = None  # per sample of the last batch: None or HistogramMatching's (k, A)
        self.last_spectral = None  # per sample of the last batch: None or FourierAdaptation's (k, strength)
        self._ms = {}

    def _mean_std(self, device):
        if device not in self._ms:
            t = torch.tensor(list(self.mean) + list(self.std), dtype=torch.float32).to(device)
            self._ms[device] = (t, t[3:])
        return self._ms[device]

    def __call__(self, images, dtype=None):
        """images: list of uint8 HWC [H_i, W_i, 3] device tensors -> [N, 3, Ho, Wo] NHWC."""
        dtype = dtype or compute_dtype()
        dev = images[0].device
        ho, wo = self.size
        out = torch.empty((len(images), 3, ho, wo), dtype=dtype, device=dev, memory_format=CL)
        ms, sd = self._mean_std(dev)
        kind = 1 if dtype == torch.bfloat16 else 0
        self.last_geometry = geometry = []
        self.last_style = styles = []
        self.last_spectral = spectrals = []
        for n, img in enumerate(images):
            img = _as_hwc_u8(img)
            h, w, c = img.shape
            ops, flip, window, flip_label, style, spectral = _sample_draws_all(self.augment, h, w)
            styles.append(style and style[1:])
            spectrals.append(spectral and spectral[1:])
            if style is not None:  # matched into a fresh image: the caller's stays as it is
                bank, k, a = style
                img = _hist_match_q8(img, image_histogram(img), bank.hist(k), a)
            if spectral is not None:  # after the matching; in place only in the pipeline's own copy
                fda, k, s = spectral
                spec, _ = band_spectrum(img, fda.band(h, w))
                img = fourier_adapt(img, spec, fda.bank.amp(k), s, out=img if style is not None else None)
            src, src_u8 = img, 1
            if window == (0, 0, h, w):  # the whole image is no window: the plain resize, for the label too
                window = None
            if window is not None or flip_label:
                geometry.append(Geometry(*(window or (0, 0, h, w)), flip_label, source=(h, w)))
            else:
                geometry.append(None)
            for t, drawn in ops:
                if isinstance(t, GaussianBlur):
                    dstf = torch.empty((h, w, c), dtype=torch.float32, device=dev)
                    _check(lib.rtsds_gaussian_blur(src.data_ptr(), src_u8, dstf.data_ptr(), c, h, w, t.kernel_size[0],
                                                   t.kernel_size[1], drawn, drawn, stream()), "gaussian blur")
                else:  # ColorJitter: in place in an fp32 intermediate, else straight from the uint8 image
                    dstf = torch.empty((h, w, c), dtype=torch.float32, device=dev) if src_u8 else src
                    color_jitter(src, *drawn, value_range=t.value_range, out=dstf)
                src, src_u8 = dstf, 0
            dst = out[n].permute(1, 2, 0)  # this image's HWC slot of the NHWC batch
            if window is None:
                ws = workspace(lib.rtsds_resize_aa_workspace(c, h, w, ho, wo), dev)
                _check(lib.rtsds_resize_aa(src.data_ptr(), src_u8, c, h, w, dst.data_ptr(), kind, ho, wo, int(flip),
                                           ms.data_ptr(), sd.data_ptr(), 0, -1, ws.data_ptr(), ws.numel(), stream()),
                       "resize")
            else:  # the blurred / jittered whole image, cut where the resize reads it
                y0, x0, hc, wc = window
                ws = workspace(lib.rtsds_resize_aa_workspace(c, hc, wc, ho, wo), dev)
                _check(lib.rtsds_crop_resize_aa(src.data_ptr(), src_u8, c, h, w, y0, x0, hc, wc, dst.data_ptr(), kind,
                                                ho, wo, int(flip), ms.data_ptr(), sd.data_ptr(), 0, -1, ws.data_ptr(),
                                                ws.numel(), stream()), "crop resize")
        return out


class LabelPipeline:
    """Resize(size, antialias=True) of an id map (interpolated in float, rounded half-to-even)
    -> optional IntRangeTransformer(lo, hi) clamp; int64 [N, 1, Ho, Wo].  With the image
    pipeline's ``last_geometry``: a sample with a window is cut and resampled nearest (no ids
    invented at region borders) straight from its uint8 / int64 source, mirrored when its flip
    was paired; a paired flip without a window mirrors the antialiased resize."""

    def __init__(self, size, clamp=None):
        self.size = (int(size[0]), int(size[1]))
        self.clamp = clamp

    def __call__(self, labels, geometry=None):
        if geometry is not None and len(geometry) != len(labels):
            raise RuntimeError(f"rtsds_amd.transforms: geometry of {len(geometry)} samples for {len(labels)} labels")
        dev = labels[0].device
        ho, wo = self.size
        out = torch.empty((len(labels), 1, ho, wo), dtype=torch.int64, device=dev)
        lo, hi = self.clamp if self.clamp is not None else (0, -1)
        for n, lab in enumerate(labels):
            lab = _as_hwc_u8(lab) if lab.dtype == torch.uint8 else lab
            geo = geometry[n] if geometry is not None else None
            flip = 0
            if geo is not None:
                if lab.dtype not in (torch.uint8, torch.int64):
                    raise RuntimeError("rtsds_amd.transforms: uint8 or int64 labels expected")
                h, w = (lab.shape[0], lab.shape[1]) if lab.dtype == torch.uint8 else (lab.shape[-2], lab.shape[-1])
                if lab.numel() != h * w:
                    raise RuntimeError("rtsds_amd.transforms: single-channel labels expected")
                y0, x0, hc, wc, flip = geo
                if getattr(geo, "source", (h, w)) != (h, w):
                    raise RuntimeError(f"rtsds_amd.transforms: label of {h} x {w} for a window drawn in an image of "
                                       f"{geo.source[0]} x {geo.source[1]}")
                if (y0, x0, hc, wc) != (0, 0, h, w):
                    lab = lab.contiguous()
                    _check(lib.rtsds_crop_resize_nearest(lab.data_ptr(), int(lab.dtype == torch.int64), h, w, y0, x0,
                                                         hc, wc, out[n].data_ptr(), ho, wo, int(flip), int(lo),
                                                         int(hi), stream()), "label crop resize")
                    continue
            if lab.dtype == torch.int64:  # decoded GTA5 ids: interpolate from a float copy
                src, u8 = lab.reshape(lab.shape[-2], lab.shape[-1], 1).float().contiguous(), 0
            else:
                src, u8 = lab, 1
            h, w = src.shape[0], src.shape[1]
            ws = workspace(lib.rtsds_resize_aa_workspace(1, h, w, ho, wo), dev)
            _check(lib.rtsds_resize_aa(src.data_ptr(), u8, 1, h, w, out[n].data_ptr(), 2, ho, wo, int(flip), None, None,
                                       int(lo), int(hi), ws.data_ptr(), ws.numel(), stream()), "label resize")
        return out


def decode_gta5_labels(rgb):
    """GTA5 RGB colour label (uint8 HWC, device) -> train ids int64 [H, W] (gta5.py:111-118)."""
    rgb = _as_hwc_u8(rgb)
    h, w = rgb.shape[0], rgb.shape[1]
    out = torch.empty((h, w), dtype=torch.int64, device=rgb.device)
    _check(lib.rtsds_gta5_decode(rgb.data_ptr(), out.data_ptr(), h, w, stream()), "gta5 decode")
    return out


def collate_raw(batch):
    """DataLoader collate for raw samples of different sizes: lists of uint8 tensors."""
    return [b[0] for b in batch], [b[1] for b in batch]


class DeviceLoader:
    """A DataLoader of raw samples -> batches ready for the network: images moved to the device
    (pinned, non-blocking) and run through ``image_pipe``, labels through ``label_pipe`` (GTA5
    colour labels decoded first when ``decode_rgb_labels``).  Same iteration / len semantics as
    the wrapped loader, so train.train / adversarial_train consume it unchanged.  An image pipe
    that records ``last_geometry`` (crop windows, paired flips) has it handed to the label pipe."""

    def __init__(self, loader, image_pipe, label_pipe, device="cuda", decode_rgb_labels=False):
        self.loader = loader
        self.image_pipe, self.label_pipe = image_pipe, label_pipe
        self.device = device
        self.decode = decode_rgb_labels
        self.epoch = 0

    def __len__(self):
        return len(self.loader)

    def _move(self, ts):
        if torch.device(self.device).type == "cpu":
            return list(ts)
        return [t.pin_memory().to(self.device, non_blocking=True) if t.device.type == "cpu" else t for t in ts]

    def __iter__(self):
        # A DistributedSampler replays the permutation of its current epoch on every iter();
        # the reference's RandomSampler draws a new one each time (adversarial_train takes
        # next(iter(loader)) per iteration, train.py:186-187), so every new iterator advances
        # the sampler's epoch.
        sampler = getattr(self.loader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(self.epoch)
            self.epoch += 1
        for images, labels in self.loader:
            images, labels = self._move(images), self._move(labels)
            if self.decode:
                labels = [decode_gta5_labels(t) for t in labels]
            x = self.image_pipe(images)
            geometry = getattr(self.image_pipe, "last_geometry", None)
            yield x, (self.label_pipe(labels) if geometry is None else self.label_pipe(labels, geometry))


def parse_size(s):
    return [int(v) for v in str(s).split(",")]


__all__ = ["ImagePipeline", "LabelPipeline", "DeviceLoader", "GaussianBlur", "RandomHorizontalFlip", "ColorJitter",
           "RandomResizedCrop", "HistogramMatching", "HistogramBank", "FourierAdaptation", "SpectrumBank", "RandomApply",
           "Geometry", "augmentation_loader", "color_jitter", "image_histogram", "histogram_match", "band_spectrum",
           "fourier_adapt", "bank_indices", "decode_gta5_labels", "collate_raw", "parse_size"]
