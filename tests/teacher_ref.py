"""Numpy restatements of the online mean-teacher kernels (rtsds_ema_step / rtsds_ema_many,
rtsds_upsample_pseudo's reduction) and of ema.EMATeacher's decay schedule.  numpy rounds every
float32 operation on its own (no FMA), which is exactly what the kernels promise."""
import math

import numpy as np


def bf16_bits(x):
    """float32 array -> the uint16 bit patterns of its bfloat16 rounding, round to nearest even
    (finite values and infinities; the tests keep NaN out of the EMA)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)


def ema_ref(t, s, w):
    """t + w * (s - t) as three separately rounded fp32 operations; returns (new t float32, its
    bf16 bit patterns)."""
    t, s, w = np.asarray(t, np.float32), np.asarray(s, np.float32), np.float32(w)
    d = np.subtract(s, t, dtype=np.float32)
    d = np.multiply(w, d, dtype=np.float32)
    out = np.add(t, d, dtype=np.float32)
    return out, bf16_bits(out)


def pseudo_ref(probs, bins, tbin=None, ignore_index=None):
    """From fp32 probabilities [..., c]: pred (uint8) = the first maximum, a NaN beating every
    number and the first NaN winning; cbin (uint16) = floor(conf * bins) clamped to
    [0, bins - 1], a conf that is not > 0 (NaN included) in bin 0; labels (int64, with ``tbin``)
    = pred where cbin >= tbin[pred], else ``ignore_index``."""
    p = np.asarray(probs, np.float32)
    c = p.shape[-1]
    flat = p.reshape(-1, c)
    pred = np.zeros(flat.shape[0], np.uint8)
    cbin = np.zeros(flat.shape[0], np.uint16)
    fb = np.float32(bins)
    for i, r in enumerate(flat):
        best, bi = r[0], 0
        for k in range(1, c):
            v = r[k]
            if v > best or (v != v and best == best):
                best, bi = v, k
        conf = np.float32(best) * np.float32(1.0)
        b = 0
        if conf > 0:
            t = np.floor(np.float32(conf * fb))
            b = bins - 1 if t >= fb else int(t)
        pred[i], cbin[i] = bi, b
    pred, cbin = pred.reshape(p.shape[:-1]), cbin.reshape(p.shape[:-1])
    labels = None
    if tbin is not None:
        tb = np.asarray(tbin, np.int64)
        labels = np.where(cbin.astype(np.int64) >= tb[pred], pred.astype(np.int64), np.int64(ignore_index))
    return pred, cbin, labels


def decay_ref(decay, updates, warmup=True):
    """The decay of update number ``updates`` (0 = the first)."""
    return min(decay, 1.0 - 1.0 / (updates + 1)) if warmup else decay


def weight_ref(decay, updates, warmup=True):
    """float32(1 - decay_t) as a Python float."""
    return float(np.float32(1.0 - decay_ref(decay, updates, warmup)))


def tbin_ref(threshold, bins):
    return int(math.ceil(threshold * bins))
