"""Numpy restatement of what rtsds_upsample_paint does with a class map: the id lookup and the
integer blend of the palette colour over the frame.  Integers only, so it is the kernel's result
bit for bit."""
import numpy as np


def ids_ref(classes, lut=None):
    """uint8 ids of a class map: lut[k], or k itself without a lut."""
    k = np.asarray(classes).astype(np.int64)
    return (k if lut is None else np.asarray(lut, np.int64)[k]).astype(np.uint8)


def paint_ref(classes, palette, alpha_q8, frame=None):
    """uint8 [..., 3]: palette[k] when alpha_q8 == 256, else
    (alpha_q8 * palette[k] + (256 - alpha_q8) * frame + 128) >> 8."""
    a = int(alpha_q8)
    assert 0 <= a <= 256
    col = np.asarray(palette, np.int64)[np.asarray(classes).astype(np.int64)]
    if a == 256:
        return col.astype(np.uint8)
    out = (a * col + (256 - a) * np.asarray(frame).astype(np.int64) + 128) >> 8
    return out.astype(np.uint8)
