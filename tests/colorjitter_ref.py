"""Plain-torch restatement of torchvision's ColorJitter forward on a float RGB image in
[0, bound] (TEST INFRASTRUCTURE; torchvision is not installed).  Generic over the dtype: every
constant takes the image's dtype, so the fp64 run is the yardstick and the fp32 run measures
what fp32 arithmetic alone costs (the tolerance of the GPU tests is 4 x that error).

    gray(p)        = 0.2989 r + 0.587 g + 0.114 b
    blend(a, b, f) = clamp(f a + (1 - f) b, 0, bound)
    id 0 brightness  blend(p, 0, fb)
    id 1 contrast    blend(p, mean over the pixels of gray(p), fc)
    id 2 saturation  blend(p, gray(p), fs)
    id 3 hue         RGB -> HSV on p / bound, h <- (h + fh) mod 1, HSV -> RGB, times bound
                     (torchvision _functional_tensor.py _rgb2hsv / _hsv2rgb)

The ids are applied in ``order``; an id whose factor is None is skipped.
"""
import itertools

import torch

ORDERS = list(itertools.permutations(range(4)))
# (fb, fc, fs, fh)
SETS = {"set1": (1.3, 0.7, 1.4, 0.1), "set2": (0.6, 1.5, 0.5, -0.3), "set3": (1.0, 1.2, 0.0, 0.5)}
SATURATING = (0.8, 1.9, 1.8, -0.5)


def gray(x):
    return 0.2989 * x[0] + 0.587 * x[1] + 0.114 * x[2]


def blend(a, b, f, bound):
    return (f * a + (1.0 - f) * b).clamp(0, bound)


def hue(x, fh, bound):
    q = x / bound
    r, g, b = q[0], q[1], q[2]
    maxc, minc = q.max(dim=0).values, q.min(dim=0).values
    eq = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eq, ones, maxc)
    crd = torch.where(eq, ones, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    mr, mg = maxc == r, maxc == g
    hr = mr * (bc - gc)
    hg = (mg & ~mr) * (2.0 + rc - bc)
    hb = (~mg & ~mr) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = (h + fh) % 1.0
    v = maxc
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p_ = (v * (1.0 - s)).clamp(0, 1)
    q_ = (v * (1.0 - f * s)).clamp(0, 1)
    t_ = (v * (1.0 - (1.0 - f) * s)).clamp(0, 1)
    table = (torch.stack([v, q_, p_, p_, t_, v]), torch.stack([t_, v, v, q_, p_, p_]),
             torch.stack([p_, p_, t_, v, v, q_]))
    return torch.stack([t.gather(0, i.unsqueeze(0)).squeeze(0) for t in table]) * bound


def color_jitter(img, order, fb, fc, fs, fh, bound=255.0):
    """img [3, H, W] float (fp32 or fp64) in [0, bound] -> the same dtype and shape."""
    x = img
    for k in order:
        if k == 0 and fb is not None:
            x = blend(x, torch.zeros_like(x), fb, bound)
        elif k == 1 and fc is not None:
            x = blend(x, gray(x).mean(), fc, bound)
        elif k == 2 and fs is not None:
            x = blend(x, gray(x).unsqueeze(0), fs, bound)
        elif k == 3 and fh is not None:
            x = hue(x, fh, bound)
    return x


def parity_image():
    """uint8 [3, 37, 53]: seeded noise, the first column band overwritten with 4x4 blocks of
    grey 128, black, white (maxc == minc and the clamps) and (200, 200, 10) (tied maxima)."""
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (3, 37, 53), generator=g, dtype=torch.uint8)
    for j, rgb in enumerate([(128, 128, 128), (0, 0, 0), (255, 255, 255), (200, 200, 10)]):
        img[:, 4 * j:4 * j + 4, 0:4] = torch.tensor(rgb, dtype=torch.uint8).view(3, 1, 1)
    return img


def random_image(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)


def refs(img, order, factors, bound=255.0):
    """(fp64 restatement, max |fp32 restatement - fp64 restatement|) of one case."""
    r64 = color_jitter(img.double(), order, *factors, bound=bound)
    r32 = color_jitter(img.float(), order, *factors, bound=bound)
    return r64, (r32.double() - r64).abs().max().item()
