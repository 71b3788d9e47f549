"""Plain-torch restatements for the paired random scale-crop (TEST INFRASTRUCTURE; torchvision
is not installed): RandomResizedCrop.get_params' draws, the nearest resample of a label window,
and the reference arithmetic of a cropped, mirrored, resized and normalised image.

get_params (torchvision transforms.RandomResizedCrop), on torch's default CPU generator:

    up to 10 times:  area share  ~ U(scale)        one uniform_
                     log ratio   ~ U(log ratio)    one uniform_
                     w = round(sqrt(area * ratio)), h = round(sqrt(area / ratio))
                     if it fits: i ~ randint(0, H - h + 1), j ~ randint(0, W - w + 1); done
    otherwise:       the largest centred window whose ratio is clamped into ``ratio``

Windows are (y0, x0, hc, wc) throughout.
"""
import math

import torch
import torch.nn.functional as F

from oracle import transforms as OT

# (source h, w; window y0, x0, hc, wc; output ho, wo): where a pitch, origin or border slip shows
AA_CASES = [
    ((64, 96), (0, 0, 64, 96), (32, 48)),        # the whole image
    ((64, 96), (0, 0, 40, 90), (48, 32)),        # down in x, up in y, top-left corner
    ((64, 96), (24, 6, 40, 90), (48, 32)),       # bottom-right corner
    ((37, 53), (5, 7, 1, 1), (4, 6)),            # a one-pixel window
    ((37, 53), (3, 2, 31, 50), (33, 17)),        # an odd non-integer scale
    ((100, 300), (10, 20, 66, 210), (33, 70)),
]
GTA_CASE = ((1052, 1914), (100, 300, 600, 1100), (720, 1280))
# (hc, wc) -> (ho, wo) of the nearest label resample
NEAREST_CASES = [((3, 5), (7, 10)), ((7, 7), (7, 7)), ((31, 53), (17, 17)), ((1, 1), (4, 4)),
                 ((600, 1100), (720, 1280))]


def get_params(h, w, scale, ratio):
    """The window and nothing else: every draw goes through the global generator."""
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    tries = 0
    while tries < 10:
        tries += 1
        share = torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect = math.exp(torch.empty(1).uniform_(lo, hi).item())
        target = share * (h * w)
        cw, ch = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if not (0 < cw <= w and 0 < ch <= h):
            continue
        top = torch.randint(0, h - ch + 1, size=(1,)).item()
        left = torch.randint(0, w - cw + 1, size=(1,)).item()
        return top, left, ch, cw
    return center_fallback(h, w, ratio)


def center_fallback(h, w, ratio):
    whole = w / h
    if whole < min(ratio):
        ch, cw = int(round(w / min(ratio))), w
    elif whole > max(ratio):
        ch, cw = h, int(round(h * max(ratio)))
    else:
        ch, cw = h, w
    return (h - ch) // 2, (w - cw) // 2, ch, cw


def inside(window, h, w):
    y0, x0, hc, wc = window
    return hc > 0 and wc > 0 and 0 <= y0 and 0 <= x0 and y0 + hc <= h and x0 + wc <= w


def nearest_label(label, window, size, flip=False, clamp=None):
    """label [H, W] integer -> int64 [ho, wo]: F.interpolate(mode="nearest") of the window, then
    the mirror, then the clamp."""
    y0, x0, hc, wc = window
    win = label[y0:y0 + hc, x0:x0 + wc]
    out = F.interpolate(win[None, None].float(), size=list(size), mode="nearest")[0, 0]
    if flip:
        out = out.flip(-1)
    out = out.long()
    return out.clamp(*clamp) if clamp is not None else out


def image_ref(img_hwc, window, size, flip, mean, std):
    """img [H, W, C] (any dtype) -> fp32 [C, ho, wo]: Normalize(Resize(flip(crop)))."""
    y0, x0, hc, wc = window
    x = img_hwc[y0:y0 + hc, x0:x0 + wc].permute(2, 0, 1).float()
    if flip:
        x = x.flip(-1)
    return OT.normalize(OT.resize(x, size), mean, std)
