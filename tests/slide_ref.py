"""Numpy restatement of the sliding-window protocol (rtsds_slide_paint, validation.sliding_windows):
the window grid, the sum over the windows covering a pixel -- ascending window index, one float32
add each -- and the first-maximum arg-max.  Ids and colours of the class map: tests/paint_ref.py."""
import numpy as np


def axis_origins(S, w, s):
    """n = ceil((S - w) / s) + 1 origins o_i = min(i * s, S - w)."""
    assert S >= w >= 1 and s >= 1
    n = (S - w + s - 1) // s + 1
    return [min(i * s, S - w) for i in range(n)]


def windows_ref(size, window, stride):
    """[(y0, x0), ...], row-major."""
    return [(y0, x0) for y0 in axis_origins(size[0], window[0], stride[0])
            for x0 in axis_origins(size[1], window[1], stride[1])]


def covering_sum(probs, table, canvas, acc=None):
    """float32 [nf, H, W, c]: ``probs[k]`` (float32 [nf, hw, ww, c], already un-mirrored) of window
    ``table[k]`` = (y0, x0, ...) summed onto the canvas in ascending k.  A pixel starts as ``acc``
    when given, else as its first covering window's value (zeros where no window covers it)."""
    nf, hw, ww, c = probs[0].shape
    H, W = canvas
    s = np.zeros((nf, H, W, c), np.float32) if acc is None else np.array(acc, np.float32)
    seen = np.full((H, W), acc is not None)
    for p, win in zip(probs, table):
        y0, x0 = win[0], win[1]
        old, first = s[:, y0:y0 + hw, x0:x0 + ww], ~seen[y0:y0 + hw, x0:x0 + ww]
        new = (old + np.asarray(p, np.float32)).astype(np.float32)
        s[:, y0:y0 + hw, x0:x0 + ww] = np.where(first[None, :, :, None], p, new)
        seen[y0:y0 + hw, x0:x0 + ww] = True
    return s


def argmax_first(s):
    """Class of each pixel: strictly greater wins, the first maximum is kept (no NaN clause)."""
    s = np.asarray(s)
    best, bi = s[..., 0].copy(), np.zeros(s.shape[:-1], np.int64)
    for k in range(1, s.shape[-1]):
        gt = s[..., k] > best
        best = np.where(gt, s[..., k], best)
        bi = np.where(gt, k, bi)
    return bi
