"""numpy restatement of the histogram matching of csrc/histmatch.hip (integers only, so the GPU
tests demand equality) and the inputs its tests share.

For one channel with source counts hs, reference counts hr, inclusive prefix sums Cs, Cr and
totals Ns, Nr:
    m[v]   = min { t in 0..255 : Cr[t] * Ns >= Cs[v] * Nr }     (v when Ns == 0 or Nr == 0)
    lut[v] = (v * (256 - A) + m[v] * A + 128) >> 8              A = strength_q8 in 0..256
    out    = lut[channel][in]
The products are taken in Python integers (no overflow to argue about)."""
import math

import numpy as np

GTA5 = (1052, 1914)


def histogram(img):
    """uint32 [3, 256] of a uint8 HWC [H, W, 3] array."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    return np.stack([np.bincount(img[..., ch].ravel(), minlength=256) for ch in range(3)]).astype(np.uint32)


def strength_q8(strength):
    return int(math.floor(strength * 256 + 0.5))


def mapping(hist_src, hist_ref):
    """m: int [3, 256], the full-strength map."""
    m = np.empty((3, 256), dtype=np.int64)
    for ch in range(3):
        cs = [int(x) for x in np.cumsum(hist_src[ch].astype(np.uint64))]
        cr = [int(x) for x in np.cumsum(hist_ref[ch].astype(np.uint64))]
        ns, nr = cs[255], cr[255]
        for v in range(256):
            if ns == 0 or nr == 0:
                m[ch, v] = v
                continue
            target = cs[v] * nr
            t = 0
            while cr[t] * ns < target:
                t += 1
            m[ch, v] = t
    return m


def lut(hist_src, hist_ref, a):
    """uint8 [3, 256]."""
    assert 0 <= a <= 256
    m = mapping(hist_src, hist_ref)
    v = np.arange(256, dtype=np.int64)[None, :]
    return ((v * (256 - a) + m * a + 128) >> 8).astype(np.uint8)


def match(img, hist_src, hist_ref, a):
    """(matched uint8 HWC image, its uint8 [3, 256] LUT)."""
    table = lut(hist_src, hist_ref, a)
    out = np.empty_like(img)
    for ch in range(3):
        out[..., ch] = table[ch][img[..., ch]]
    return out, table


def cdf_distance(img, hist_ref):
    """Mean over channels and values of |CDF(img) - CDF(reference)|."""
    h = histogram(img).astype(np.float64)
    r = hist_ref.astype(np.float64)
    return float(np.abs(np.cumsum(h, 1) / h.sum(1, keepdims=True) - np.cumsum(r, 1) / r.sum(1, keepdims=True)).mean())


# ------------------------------------------------------------------ inputs
def skewed(h, w, seed, g):
    return (255 * np.random.default_rng(seed).random((h, w, 3)) ** g).astype(np.uint8)


def source(h=64, w=96, seed=1):
    """Dark-heavy (gamma 2.2)."""
    return skewed(h, w, seed, 2.2)


def reference(h=37, w=53, seed=2):
    """Bright-heavy (gamma 0.5), of another size than the source: Ns != Nr."""
    return skewed(h, w, seed, 0.5)


def noise(h, w, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def constant(h, w, rgb=(17, 200, 255)):
    return np.broadcast_to(np.array(rgb, dtype=np.uint8), (h, w, 3)).copy()


def two_valued(h, w, seed=4, lo=3, hi=250):
    pick = np.random.default_rng(seed).random((h, w, 3)) < 0.3
    return np.where(pick, np.uint8(hi), np.uint8(lo)).astype(np.uint8)


def ramp(h, w):
    """Horizontal ramp over the full range, the channels shifted against each other."""
    x = (np.arange(w, dtype=np.int64) * 255 // max(w - 1, 1))[None, :, None]
    return np.broadcast_to((x + np.array([0, 85, 170])) % 256, (h, w, 3)).astype(np.uint8)


def sky(h, w, seed=5, value=(135, 180, 235)):
    """70 % of the pixels at one value (most lanes of a wave on one bin), the rest noise."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[rng.random((h, w)) < 0.7] = np.array(value, dtype=np.uint8)
    return img


def midband(h, w, seed=6):
    """Values in 40..199 only: empty bins at both ends."""
    return np.random.default_rng(seed).integers(40, 200, (h, w, 3), dtype=np.uint8)
