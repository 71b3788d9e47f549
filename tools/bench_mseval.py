"""Micro-benchmark of the multi-scale / flip probability accumulation (rtsds_upsoftmax_acc) at
the evaluation geometry: 12 passes (scales 0.5 .. 1.75, each plain and mirrored) of a
[8, 19, h/8, w/8] head to 512 x 1024, in bf16 and fp32, against the same job built from the
unfused ops (upsample_softmax -> .float() -> torch.flip -> add, then argmax_channels).

    python tools/bench_mseval.py [reps=50] [rounds=3]

Times are HIP events around ``reps`` back-to-back jobs, after a warm-up of every shape; the
fused and the unfused job alternate ``rounds`` times and the median round is reported.  GB/s is
the algorithmic traffic of the fused kernel (low-res head read, 4c B/px of acc read on all but
the first pass, 4c B/px written, 8 B/px of pred on the last pass) over its time."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd.validation import scaled_size  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
assert torch.cuda.is_available(), "bench_mseval needs a HIP device"
dev = "cuda"
N, C, SIZE = 8, 19, (512, 1024)
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E specification


def timed(job):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        job()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps  # ms per 12-pass job


for dt in (torch.bfloat16, torch.float32):
    g = torch.Generator().manual_seed(0)
    lows = []
    for s in SCALES:
        h, w = scaled_size(SIZE, s)
        lows.append((torch.randn(N, C, h // 8, w // 8, generator=g) * 3).to(dev, dt)
                    .contiguous(memory_format=torch.channels_last))
    passes = [(x, F.upsample_geometry(x, size=SIZE), flip) for x in lows for flip in (False, True)]
    acc = torch.empty((N, *SIZE, C), dtype=torch.float32, device=dev)
    pred = torch.empty((N, *SIZE), dtype=torch.int64, device=dev)

    def fused():
        for i, (x, geo, flip) in enumerate(passes):
            F.upsample_softmax_accumulate(x, geo, acc, flip=flip, accumulate=i > 0,
                                          pred=pred if i == len(passes) - 1 else None)
        return acc, pred

    def chain():
        total = None
        for x, geo, flip in passes:
            p = F.upsample_softmax(x, geo).float()
            if flip:
                p = torch.flip(p, dims=[3])
            total = p if total is None else total.add_(p)
        return total, F.argmax_channels(total)

    # the two jobs agree (fp32: bit for bit; bf16: the chain rounds every probability to bf16)
    a, p = fused()
    t, q = chain()
    diff = (a - t.permute(0, 2, 3, 1)).abs().max().item()
    assert diff == 0.0 if dt == torch.float32 else diff <= len(passes) * 2.0 ** -9, diff
    del a, p, t, q
    for _ in range(3):
        fused()
        chain()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(rounds):
        tf.append(timed(fused))
        tc.append(timed(chain))
    px = N * SIZE[0] * SIZE[1]
    nbytes = sum(x.numel() * x.element_size() for x, _, _ in passes) + px * (4 * C * (2 * len(passes) - 1) + 8)
    mf, mc = statistics.median(tf), statistics.median(tc)
    gbs = nbytes / (mf * 1e-3) / 1e9
    print(json.dumps({"dtype": str(dt).split(".")[-1], "passes": len(passes), "reps": reps, "rounds": rounds,
                      "fused_ms": round(mf, 4), "chain_ms": round(mc, 4), "ratio": round(mc / mf, 3),
                      "fused_ms_rounds": [round(v, 4) for v in tf], "chain_ms_rounds": [round(v, 4) for v in tc],
                      "fused_bytes": nbytes, "fused_GBps": round(gbs, 1),
                      "hbm_peak_fraction": round(gbs * 1e9 / HBM_PEAK, 3), "max_abs_diff": diff}))
    assert all(f < c for f, c in zip(tf, tc)), "fused accumulation slower than the unfused chain"
