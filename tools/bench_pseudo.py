"""Micro-benchmark of pseudo-label generation (rtsds_conf_hist + rtsds_pseudo_select) at the
self-training geometry: acc = [8, 512, 1024, 19] fp32, 1024 bins, against the same job built
from torch ops on the same device (max over classes, multiply, floor, clamp, bincount of
class * bins + bin added to the histogram, the uint8 / int16 copies of class and bin, then
``where`` against the per-class thresholds).

    python tools/bench_pseudo.py [reps=30] [bins=1024]

Two inputs: ``softmax`` (sum of two softmaxes of 3 * randn logits: confidences spread over all
bins) and ``one_hot`` (every pixel class 3 at confidence 1.0: all 4.2 M pixels land in ONE
histogram cell, the worst case for the LDS atomics).  Each repetition is timed with its own pair
of HIP events after a warm-up; the kernels and the chain alternate and the median is reported.
GB/s is the algorithmic traffic of the two kernels -- 4c B/px of acc read, 3 B/px of (pred, cbin)
written, 3 B/px read back and 8 B/px of labels written: 79 + 11 B/px at 19 classes, reported
for the histogram kernel alone (79 B/px) and for the pair."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rtsds_amd import functional as F  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
assert reps >= 20, "at least 20 timed repetitions"
assert torch.cuda.is_available(), "bench_pseudo needs a HIP device"
dev = "cuda"
N, H, W, C, PASSES, IGNORE = 8, 512, 1024, 19, 2, 19
BINS = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E specification
px = N * H * W


def inputs():
    g = torch.Generator(device=dev).manual_seed(0)
    acc = torch.zeros((N, H, W, C), dtype=torch.float32, device=dev)
    for _ in range(PASSES):
        acc += torch.softmax(3 * torch.randn((N, H, W, C), generator=g, device=dev), dim=-1)
    yield "softmax", acc
    acc = torch.zeros((N, H, W, C), dtype=torch.float32, device=dev)
    acc[..., 3] = PASSES
    yield "one_hot", acc


def timed(job):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    job()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3  # us


for name, acc in inputs():
    tbin = torch.randint(BINS // 2, BINS, (C,), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
    hist = torch.zeros((C, BINS), dtype=torch.int64, device=dev)
    pred = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    cbin = torch.empty((N, H, W), dtype=torch.uint16, device=dev)
    lab = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    hist_c = torch.zeros((C, BINS), dtype=torch.int64, device=dev)
    inv = 1.0 / PASSES
    tbin64 = tbin.long()
    kept = {}

    def hist_only():
        F.confidence_histogram(acc, hist, passes=PASSES, pred=pred, cbin=cbin)

    def kernels():
        F.confidence_histogram(acc, hist, passes=PASSES, pred=pred, cbin=cbin)
        F.pseudo_select(pred, cbin, tbin, IGNORE, out=lab)

    def chain():
        conf, k = acc.max(dim=-1)
        b = torch.floor(conf * inv * BINS).clamp_(0, BINS - 1).long()
        hist_c.add_(torch.bincount((k * BINS + b).view(-1), minlength=C * BINS).view(C, BINS))
        kept["pred"], kept["cbin"] = k.to(torch.uint8), b.to(torch.int16)
        kept["lab"] = torch.where(b >= tbin64[k], k, IGNORE)

    # the two jobs agree (integer results; the softmax input has no ties between classes)
    kernels()
    chain()
    torch.cuda.synchronize()
    assert torch.equal(hist, hist_c) and torch.equal(lab, kept["lab"]) and torch.equal(pred, kept["pred"])
    for _ in range(5):
        kernels()
        chain()
        hist_only()
    torch.cuda.synchronize()
    tk, tc, th = [], [], []
    for _ in range(reps):
        tk.append(timed(kernels))
        tc.append(timed(chain))
        th.append(timed(hist_only))
    mk, mc, mh = statistics.median(tk), statistics.median(tc), statistics.median(th)
    q = lambda v: [round(x, 1) for x in statistics.quantiles(v, n=10)[::8]]  # noqa: E731  (10 % / 90 %)
    hist_bytes, pair_bytes = px * (4 * C + 3), px * (4 * C + 3 + 3 + 8)
    print(json.dumps({"input": name, "shape": [N, H, W, C], "bins": BINS, "reps": reps,
                      "kernels_us": round(mk, 1), "kernels_us_p10_p90": q(tk),
                      "conf_hist_us": round(mh, 1), "conf_hist_us_p10_p90": q(th),
                      "chain_us": round(mc, 1), "chain_us_p10_p90": q(tc), "ratio": round(mc / mk, 2),
                      "conf_hist_GBps_at_79B_px": round(hist_bytes / (mh * 1e-6) / 1e9, 1),
                      "pair_GBps": round(pair_bytes / (mk * 1e-6) / 1e9, 1),
                      "conf_hist_hbm_peak_fraction": round(hist_bytes / (mh * 1e-6) / HBM_PEAK, 3)}))
    assert mk < mc, f"{name}: the kernels ({mk:.1f} us) do not beat the torch chain ({mc:.1f} us)"
