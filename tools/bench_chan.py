"""Micro-benchmark of chan.hip's per-pixel class kernels at the workload's shape ([8, 19, 512, 1024]
logits: channel softmax forward / backward, cross-entropy forward / backward, argmax) for library
A/B runs:
    RTSDS_LIB=... python tools/bench_chan.py OUT.json
Times the LDS-staged route (NHWC, bf16 and fp32) and the strided route (NCHW, fp32) through the C
ABI with device events, and saves one SHA-256 per output (the tensors are up to 318 MB each) so two
libraries can be compared bit for bit."""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rtsds_amd._lib import BF16, F32, lib  # noqa: E402

N, C, H, W = 8, 19, 512, 1024
HW, IGNORE, WARM, ITERS = H * W, 19, 3, 20
dev = "cuda"
st = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cpu").manual_seed(5)
out = {}


def timed(name, fn):
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print(f"{name:44s} {e0.elapsed_time(e1) / ITERS * 1e3:8.1f} us")


def keep(name, t):
    out[name] = hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


tgt = torch.randint(0, 20, (N, H, W), generator=g).to(dev)  # 19 = ignore_index
for tag, dt, tdt, nchw in (("staged bf16", BF16, torch.bfloat16, False), ("staged fp32", F32, torch.float32, False),
                           ("strided fp32 NCHW", F32, torch.float32, True)):
    x = (torch.randn(N, H, W, C, generator=g) * 3).to(dev, tdt)
    dy = torch.randn(N, H, W, C, generator=g).to(dev, tdt)
    sn, sc, shw = (C * HW, HW, 1) if nchw else (HW * C, 1, C)
    if nchw:
        x = x.permute(0, 3, 1, 2).contiguous()
    y, dx, dxce = torch.empty(N, H, W, C, device=dev, dtype=tdt), torch.empty_like(x), torch.empty_like(x)
    ws = torch.zeros(lib.rtsds_ce_workspace() // 4, device=dev)
    loss, gl = torch.zeros(1, device=dev), torch.ones(1, device=dev)
    am = torch.empty(N, H, W, device=dev, dtype=torch.int64)
    correct = torch.zeros(1, device=dev, dtype=torch.int64)
    P = torch.Tensor.data_ptr
    timed(f"{tag}: softmax fwd", lambda: lib.rtsds_softmax_fwd(P(x), sn, sc, shw, P(y), C, N, HW, C, dt, st))
    timed(f"{tag}: softmax bwd", lambda: lib.rtsds_softmax_bwd(P(dy), P(y), C, P(dx), sn, sc, shw, N, HW, C, dt, st))
    timed(f"{tag}: cross-entropy fwd", lambda: lib.rtsds_ce_fwd(P(x), sn, sc, shw, P(tgt), P(loss), N, HW, C, IGNORE, dt, P(ws),
                                                               ws.numel() * 4, st))
    timed(f"{tag}: cross-entropy bwd", lambda: lib.rtsds_ce_bwd(P(x), sn, sc, shw, P(tgt), P(gl), P(ws) + 2048 * 4, P(dxce), N, HW,
                                                               C, IGNORE, dt, st))
    timed(f"{tag}: argmax", lambda: lib.rtsds_argmax(P(x), sn, sc, shw, P(am), P(tgt), P(correct), N, HW, C, dt, st))
    for name, t in (("y", y), ("dx", dx), ("loss", loss), ("ws", ws), ("dx_ce", dxce), ("argmax", am), ("correct", correct)):
        keep(f"{tag} {name}", t)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
