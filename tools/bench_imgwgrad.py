"""Times the weight gradient of the 3-channel stride-2 image convs behind a train-mode BatchNorm
at the bench geometries through the C ABI: the separate passes (rtsds_bn_bwd writing dx, then
rtsds_conv2d_wgrad) against the fused form (rtsds_bn_bwd_coef, then rtsds_imgconv_bn_wgrad), for
the ResNet stem (7x7 s2 p3) and the spatial-path conv (3x3 s2 p1), input in the 4-channel pitch
(pack_input).  usage: bench_imgwgrad.py [N H W] [iters]"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd._lib import BF16, INPUT_PADDED, lib  # noqa: E402
from rtsds_amd.runtime import workspace  # noqa: E402

n, h, w = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (8, 512, 1024)
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 30
dev = "cuda"
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
st = torch.cuda.current_stream().cuda_stream
x = F.pack_input(torch.randn(n, 3, h, w, device=dev), torch.bfloat16)


def timed(fn):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


for kh, pad in ((7, 3), (3, 1)):
    d = F._conv_desc(x, 64, kh, kh, (2, 2), (pad, pad), (1, 1))
    rows = d.n * d.ho * d.wo
    bx = torch.randn(rows, 64, device=dev).to(torch.bfloat16)
    g = torch.randn(rows, 64, device=dev).to(torch.bfloat16)
    dx = torch.empty_like(bx)
    gamma, beta = torch.rand(64, device=dev) + 0.5, torch.randn(64, device=dev)
    sm = bx.float().mean(0).contiguous()
    si = (1.0 / torch.sqrt(bx.float().var(0, unbiased=False) + 1e-5)).contiguous()
    dg, db, coef = torch.empty(64, device=dev), torch.empty(64, device=dev), torch.empty(6 * 64, device=dev)
    dw = torch.zeros(64, kh, kh, 3, device=dev)
    wsb = workspace(lib.rtsds_bn_workspace(rows, 64), x.device)
    wsw = workspace(lib.rtsds_conv2d_wgrad_workspace(ctypes.byref(d)), x.device)
    wsf = workspace(lib.rtsds_imgconv_bn_wgrad_workspace(ctypes.byref(d)), x.device)
    bn = lambda: lib.rtsds_bn_bwd(P(g), P(bx), None, P(dx), None, P(dg), P(db), rows, 64, P(gamma), P(beta), P(sm), P(si),  # noqa: E731
                                  1, 1, 0, BF16, P(wsb), wsb.numel(), st)
    wg = lambda: lib.rtsds_conv2d_wgrad(ctypes.byref(d), P(x), P(dx), P(dw), None, INPUT_PADDED, P(wsw), wsw.numel(), st)  # noqa: E731
    cf = lambda: lib.rtsds_bn_bwd_coef(P(g), P(bx), P(dg), P(db), P(coef), rows, 64, P(gamma), P(beta), P(sm), P(si),  # noqa: E731
                                       1, 1, 0, BF16, P(wsb), wsb.numel(), st)
    fu = lambda: lib.rtsds_imgconv_bn_wgrad(ctypes.byref(d), P(x), P(g), P(bx), P(coef), 1, P(dw), INPUT_PADDED, P(wsf),  # noqa: E731
                                            wsf.numel(), st)
    t = [timed(f) for f in (bn, wg, cf, fu)]
    mb = (2 * bx.numel() * 2 + x.numel() // 3 * 4 * 2) / 1e6
    print(f"k{kh} separate: bn_bwd {t[0]:6.1f} + wgrad {t[1]:6.1f} = {t[0] + t[1]:6.1f} us | fused: bn_bwd_coef {t[2]:6.1f} + "
          f"bn_wgrad {t[3]:6.1f} = {t[2] + t[3]:6.1f} us (g + x + image {mb:.0f} MB: {mb / t[3]:.2f} TB/s incl. the slab reduce)",
          flush=True)
