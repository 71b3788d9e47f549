"""Micro-benchmark of the online mean-teacher hot pieces against their unfused counterparts, timed
in the same run:

(a) labels: functional.upsample_pseudo (rtsds_upsample_pseudo, one launch) against the
    three-kernel chain it replaces, upsample_softmax_accumulate(accumulate=False) ->
    confidence_histogram(passes=1, pred, cbin) -> pseudo_select, at N = 4, 64 x 128 -> 512 x 1024,
    19 classes, bf16 head, 1024 bins;
(b) teacher update: one EMATeacher.update() on BiSeNet-R18 (one rtsds_ema_step per arena with the
    bf16 shadow written in the same pass, one rtsds_ema_many over the BatchNorm statistics)
    against torch._foreach_lerp_ over the same parameters and statistics plus the bf16 re-cast
    of the conv weights.

    python tools/bench_teacher.py [reps=30] [calls=20]

Each repetition times ``calls`` back-to-back calls of one job between a pair of HIP events (a
single call is a few tens of microseconds); the jobs alternate after a warm-up and the median
per-call time with the 10 % / 90 % quantiles is reported, one JSON line per piece.  B/px counts
the algorithmic traffic at full resolution: the chain writes and re-reads the fp32 probabilities
(2 x 4c), writes and re-reads pred / cbin (2 x 3) and writes the labels (8); the fused kernel
writes the labels only."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rtsds_amd  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import optim  # noqa: E402
from rtsds_amd.ema import EMATeacher  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
assert reps >= 20, "at least 20 timed repetitions"
assert torch.cuda.is_available(), "bench_teacher needs a HIP device"
dev = "cuda"


def timed(job):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        job()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / calls  # us per call


def compare(fused, unfused):
    for _ in range(5):
        fused()
        unfused()
    torch.cuda.synchronize()
    tf, tu = [], []
    for _ in range(reps):
        tf.append(timed(fused))
        tu.append(timed(unfused))
    q = lambda v: [round(x, 1) for x in statistics.quantiles(v, n=10)[::8]]  # noqa: E731  (10 % / 90 %)
    return statistics.median(tf), q(tf), statistics.median(tu), q(tu)


# ----------------------------------------------------------------------------- (a) labels
N, HI, WI, H, W, C, BINS, IGNORE = 4, 64, 128, 512, 1024, 19, 1024, 19
g = torch.Generator(device=dev).manual_seed(0)
low = (3 * torch.randn((N, HI, WI, C), generator=g, device=dev)).to(torch.bfloat16).permute(0, 3, 1, 2)
geo = F.upsample_geometry(low, size=(H, W))
tbin = torch.full((C,), int(np.ceil(0.5 * BINS)), dtype=torch.int32, device=dev)
acc = torch.empty((N, H, W, C), dtype=torch.float32, device=dev)
hist = torch.zeros((C, BINS), dtype=torch.int64, device=dev)
pred = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
cbin = torch.empty((N, H, W), dtype=torch.uint16, device=dev)
lab_c = torch.empty((N, H, W), dtype=torch.int64, device=dev)
lab_f = torch.empty((N, H, W), dtype=torch.int64, device=dev)
pred_f, cbin_f = torch.empty_like(pred), torch.empty_like(cbin)


def fused_labels():
    F.upsample_pseudo(low, geo, BINS, tbin=tbin, ignore_index=IGNORE, labels=lab_f)


def fused_pred_cbin():
    F.upsample_pseudo(low, geo, BINS, pred=pred_f, cbin=cbin_f)


def chain():
    F.upsample_softmax_accumulate(low, geo, acc, accumulate=False)
    F.confidence_histogram(acc, hist, passes=1, pred=pred, cbin=cbin)
    F.pseudo_select(pred, cbin, tbin, IGNORE, out=lab_c)


fused_labels()
fused_pred_cbin()
chain()
torch.cuda.synchronize()
assert torch.equal(lab_f, lab_c) and torch.equal(pred_f, pred) and torch.equal(cbin_f.view(torch.int16), cbin.view(torch.int16))
share = float((lab_f != IGNORE).float().mean())
px = N * H * W
low_bytes = N * HI * WI * C * 2
mf, qf, mc, qc = compare(fused_labels, chain)
mp, qp, _, _ = compare(fused_pred_cbin, chain)
print(json.dumps({"piece": "labels", "shape": [N, HI, WI, C], "to": [H, W], "dtype": "bf16", "bins": BINS, "reps": reps,
                  "calls_per_rep": calls, "labelled_share": round(share, 3),
                  "fused_labels_us": round(mf, 1), "fused_labels_us_p10_p90": qf,
                  "fused_pred_cbin_us": round(mp, 1), "fused_pred_cbin_us_p10_p90": qp,
                  "chain_us": round(mc, 1), "chain_us_p10_p90": qc, "ratio": round(mc / mf, 2),
                  "fused_B_px": 8, "chain_B_px": 8 * C + 6 + 8,
                  "fused_GBps": round((px * 8 + low_bytes) / (mf * 1e-6) / 1e9, 1),
                  "chain_GBps": round((px * (8 * C + 14) + low_bytes) / (mc * 1e-6) / 1e9, 1)}))
labels_ok = mf < mc

# ----------------------------------------------------------------------------- (b) teacher update
student = BiSeNet(19, "resnet18").to(dev).train()
opt = optim.Adam(student.parameters(), lr=1e-4)
teacher = EMATeacher(student, BiSeNet(19, "resnet18").to(dev), opt, decay=0.99, warmup=False)
w = teacher.weight()
# the unfused counterpart works on a third model of its own: per-tensor lerp + bf16 cast of the weights
other = BiSeNet(19, "resnet18").to(dev).eval()
sp = dict(student.named_parameters())
sb = dict(student.named_buffers())
t_float = [p.data for _, p in other.named_parameters()] + [b for _, b in other.named_buffers() if b.is_floating_point()]
s_float = [sp[k].data for k, _ in other.named_parameters()] + [sb[k] for k, b in other.named_buffers() if b.is_floating_point()]
ints = [(b, sb[k]) for k, b in other.named_buffers() if not b.is_floating_point()]
weights = [p.data for p in other.parameters() if p.dim() == 4]
shadows = [torch.empty_like(x, dtype=torch.bfloat16) for x in weights]
elements = sum(t.numel() for t in t_float)


def fused_update():
    teacher.update()


def foreach_update():
    torch._foreach_lerp_(t_float, s_float, w)
    for x, h in zip(weights, shadows):
        h.copy_(x)
    torch._foreach_copy_([t for t, _ in ints], [s for _, s in ints])


with torch.no_grad(), rtsds_amd.precision(torch.bfloat16):
    mf, qf, mu, qu = compare(fused_update, foreach_update)
launches = len(teacher._store) + 1  # + the batched copy of the integer buffers on both sides
print(json.dumps({"piece": "teacher_update", "model": "BiSeNet-R18", "elements": elements, "reps": reps, "calls_per_rep": calls,
                  "fused_update_us": round(mf, 1), "fused_update_us_p10_p90": qf, "fused_launches": launches,
                  "foreach_lerp_cast_us": round(mu, 1), "foreach_lerp_cast_us_p10_p90": qu,
                  "unfused_tensors": len(t_float), "unfused_casts": len(weights), "ratio": round(mu / mf, 2),
                  "fused_GBps_at_14B_el": round(elements * 14 / (mf * 1e-6) / 1e9, 1)}))
assert labels_ok, "upsample_pseudo does not beat the three-kernel chain"
assert mf < mu, f"EMATeacher.update() ({mf:.1f} us) does not beat foreach_lerp + casts ({mu:.1f} us)"
