"""float64 restatement of class-weighted cross-entropy after a bilinear upsample, shared by
tests/test_wce_cpu.py (which checks it against torch's own fp64 chain) and tests/test_wce_gpu.py
(which checks the HIP kernels against it).  Closed forms only, no autograd:

    up_h   = Ry @ head_h @ Rx^T                      (bilinear, align_corners=False, ATen's rule)
    loss_h = sum_valid w[t] (lse(z) - z[t]) / sum_valid w[t]
    dz     = w[t] / sum_valid w * (softmax(z) - onehot(t))       (0 on ignored pixels)
    dhead  = Ry^T @ dz @ Rx

Importable without a device.  Every case and its data are built once (lru_cache) and never changed."""
import functools
from collections import namedtuple

import numpy as np
import torch

IGNORE = 255
# (n, c, hl, wl, resize, heads[, logit amplitude]): one planning branch of the fused kernel each
CASES = [
    (2, 19, 8, 16, {"scale_factor": 8}, 3),         # bench form, auxiliary wave
    (1, 19, 13, 17, {"size": (97, 129)}, 2),        # non-integer ratio, ragged tiles
    (2, 5, 7, 9, {"scale_factor": 4}, 1),           # runtime c
    (2, 19, 8, 16, {"scale_factor": 2}, 3),         # no auxiliary wave: LDS cap
    (2, 19, 8, 16, {"scale_factor": 2}, 2),         # auxiliary wave at the same geometry
    (1, 19, 16, 40, {"scale_factor": 3}, 1),        # narrowed tile width, several column tiles
    (2, 19, 8, 16, {"scale_factor": 8}, 2, 40.0),   # softmax shift, far-class underflow
    (1, 32, 5, 6, {"scale_factor": 8}, 4),          # largest c, four heads, no spare wave
]
IDS = [f"n{c[0]}c{c[1]}_{c[2]}x{c[3]}_{'x%d' % c[4]['scale_factor'] if 'scale_factor' in c[4] else 'to%dx%d' % c[4]['size']}"
       f"_k{c[5]}{'_amp%d' % c[6] if len(c) > 6 else ''}" for c in CASES]

Data = namedtuple("Data", "heads target weight H W sh sw")


def out_size(hl, wl, resize):
    """(H, W, scale_h, scale_w): torch's rule -- scale_factor form maps with 1 / scale_factor."""
    if "scale_factor" in resize:
        f = resize["scale_factor"]
        return int(np.floor(hl * f)), int(np.floor(wl * f)), 1.0 / f, 1.0 / f
    H, W = resize["size"]
    return H, W, hl / H, wl / W


def weights_for(c, seed=3):
    """Uniform in [0.25, 4], rounded to fp32, one class set to 0."""
    g = torch.Generator().manual_seed(seed)
    w = (0.25 + 3.75 * torch.rand(c, generator=g, dtype=torch.float64)).float()
    w[c // 2] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _data(idx, bf16):
    n, c, hl, wl, resize, k = CASES[idx][:6]
    amp = CASES[idx][6] if len(CASES[idx]) > 6 else 2.0
    g = torch.Generator().manual_seed(21 + idx)
    heads = [torch.randn(n, c, hl, wl, generator=g, dtype=torch.float64) * amp for _ in range(k)]
    if bf16:
        heads = [h.bfloat16().double() for h in heads]
    H, W, sh, sw = out_size(hl, wl, resize)
    t = torch.randint(0, c + 1, (n, H, W), generator=g)
    t[t == c] = IGNORE
    return Data(tuple(heads), t, weights_for(c), H, W, sh, sw)


def data(idx, bf16=False):
    """Case ``idx``'s inputs: fp64 heads (bf16-representable when ``bf16``), int64 target with the
    ignore value 255, fp32 weights."""
    return _data(idx, bool(bf16))


def _taps(n_out, n_in, scale):
    """[n_out, n_in] interpolation matrix, align_corners=False (ATen area_pixel_compute_source_index)."""
    R = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        src = max((o + 0.5) * scale - 0.5, 0.0)
        i0 = min(int(np.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l1 = src - i0
        R[o, i0] += 1.0 - l1
        R[o, i1] += l1
    return R


def upsample(head, H, W, sh, sw):
    Ry, Rx = _taps(H, head.shape[2], sh), _taps(W, head.shape[3], sw)
    return torch.einsum("yi,ncij,xj->ncyx", Ry, head.double(), Rx)


def weighted_ce(z, t, w, ignore=IGNORE, gout=1.0):
    """Full-resolution logits z [n, c, H, W] (fp64) -> (loss, dz, weight sum); w None: unweighted."""
    n, c = z.shape[:2]
    w = torch.ones(c, dtype=torch.float64) if w is None else w.double()
    valid = t != ignore
    tc = torch.where(valid, t, torch.zeros_like(t))
    wt = torch.where(valid, w[tc], torch.zeros((), dtype=torch.float64))
    m = z.max(1, keepdim=True).values
    e = torch.exp(z - m)
    se = e.sum(1, keepdim=True)
    lse = (torch.log(se) + m).squeeze(1)
    zt = z.gather(1, tc.unsqueeze(1)).squeeze(1)
    wsum = wt.sum()
    loss = (wt * (lse - zt)).sum() / wsum
    onehot = torch.zeros_like(z).scatter_(1, tc.unsqueeze(1), 1.0)
    dz = (gout * wt / wsum).unsqueeze(1) * (e / se - onehot)
    return loss, dz, wsum


def fused_reference(heads, t, w, H, W, sh, sw, ignore=IGNORE, gout=1.0):
    """(sum of the heads' losses, [d loss / d head], head 0's full-resolution logits)."""
    total, grads, up0 = 0.0, [], None
    for h in heads:
        Ry, Rx = _taps(H, h.shape[2], sh), _taps(W, h.shape[3], sw)
        z = torch.einsum("yi,ncij,xj->ncyx", Ry, h.double(), Rx)
        up0 = z if up0 is None else up0
        loss, dz, _ = weighted_ce(z, t, w, ignore, gout)
        total = total + loss
        grads.append(torch.einsum("yi,ncyx,xj->ncij", Ry, dz, Rx))
    return total, grads, up0


@functools.lru_cache(maxsize=None)
def reference(idx, bf16=False, gout=1.5):
    d = data(idx, bf16)
    return fused_reference(d.heads, d.target, d.weight, d.H, d.W, d.sh, d.sw, IGNORE, gout)


def label_stats(labels, c, ignore):
    """(count, support) of functional.label_stats with numpy.bincount per image."""
    count = np.zeros(c, dtype=np.int64)
    support = np.zeros(c, dtype=np.int64)
    for img in np.asarray(labels).reshape(labels.shape[0], -1):
        ok = img[(img != ignore) & (img >= 0) & (img < c)]
        b = np.bincount(ok, minlength=c).astype(np.int64)
        count += b
        support += np.where(b > 0, ok.size, 0)
    return count, support
