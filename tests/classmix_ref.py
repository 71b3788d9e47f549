"""Numpy restatement of ClassMix as rtsds_class_presence / rtsds_classmix define it (TEST
INFRASTRUCTURE).  Everything is an integer or a byte copy, so the GPU results must EQUAL these.

Per sample n, with the window win = slab[n, y0:y0+H, x0:x0+W] of the int64 source labels and c
classes (a label s is a class iff 0 <= s < c):

    present[n]  bit k set iff some window pixel equals class k
    chosen[n]   P = classes of present[n], m = (|P| + 1) >> 1; class k of P is chosen iff
                #{j in P : perm[n, j] < perm[n, k] or (perm[n, j] == perm[n, k] and j < k)} < m
    M           win is a class and that class is chosen
    out_img     M ? the source window's pixel record : the target's      (whole records, as bytes)
    out_lab     M ? win : (pred < c and cbin >= tbin[pred] ? pred : ignore_index)

Images are raw byte arrays [N, H, W, pix_bytes] (the pad lane of a 4-element pitch included).
"""
import numpy as np


def presence(slab, size, origins, c):
    """uint32 [N] from int64 slab [N, Hs, Ws], size (H, W), origins [N, 2] rows (y0, x0)."""
    h, w = size
    out = np.zeros(slab.shape[0], dtype=np.uint32)
    for n in range(slab.shape[0]):
        y0, x0 = int(origins[n][0]), int(origins[n][1])
        assert 0 <= y0 <= slab.shape[1] - h and 0 <= x0 <= slab.shape[2] - w
        win = slab[n, y0:y0 + h, x0:x0 + w]
        bits = 0
        for k in np.unique(win):
            if 0 <= k < c:
                bits |= 1 << int(k)
        out[n] = bits
    return out


def choose(present, perm, c):
    """The chosen-class mask (python int) of one sample from its presence mask and key row."""
    p = [k for k in range(c) if (int(present) >> k) & 1]
    m = (len(p) + 1) >> 1
    chosen = 0
    for k in p:
        before = sum(1 for j in p if perm[j] < perm[k] or (perm[j] == perm[k] and j < k))
        if before < m:
            chosen |= 1 << k
    return chosen


def pseudo(pred, cbin, tbin, ignore_index):
    """rtsds_pseudo_select's rule on integer numpy arrays (pred may hold values >= c)."""
    pred, cbin, tbin = pred.astype(np.int64), cbin.astype(np.int64), np.asarray(tbin).astype(np.int64)
    c = tbin.shape[0]
    valid = pred < c
    thr = tbin[np.where(valid, pred, 0)]
    return np.where(valid & (cbin >= thr), pred, ignore_index).astype(np.int64)


def classmix(src, slab, tgt, pred, cbin, tbin, perm, origins, ignore_index):
    """src uint8 [N, Hs, Ws, pix], slab int64 [N, Hs, Ws], tgt uint8 [N, H, W, pix], pred / cbin
    integer [N, H, W], tbin [c], perm [N, c], origins [N, 2].  Returns a dict: out_img (uint8
    [N, H, W, pix]), out_lab (int64), mask (uint8), present, chosen (uint32 [N])."""
    n, h, w, pix = tgt.shape
    c = len(tbin)
    assert src.shape[0] == n and src.shape[3] == pix and slab.shape == src.shape[:3]
    present = presence(slab, (h, w), origins, c)
    chosen = np.array([choose(present[i], [int(v) for v in perm[i]], c) for i in range(n)], dtype=np.uint32)
    plab = pseudo(pred, cbin, tbin, ignore_index)
    out_img, out_lab = np.empty_like(tgt), np.empty((n, h, w), np.int64)
    mask = np.empty((n, h, w), np.uint8)
    for i in range(n):
        y0, x0 = int(origins[i][0]), int(origins[i][1])
        win = slab[i, y0:y0 + h, x0:x0 + w]
        is_class = (win >= 0) & (win < c)
        lut = np.array([(int(chosen[i]) >> k) & 1 for k in range(c)], dtype=bool)
        m = is_class & lut[np.where(is_class, win, 0)]
        out_img[i] = np.where(m[..., None], src[i, y0:y0 + h, x0:x0 + w], tgt[i])
        out_lab[i] = np.where(m, win, plab[i])
        mask[i] = m
    return {"out_img": out_img, "out_lab": out_lab, "mask": mask, "present": present, "chosen": chosen}
