"""Class-weighted cross-entropy timing (profiles/wce/README.md), bare ctypes calls on
preallocated buffers, each call timed by its own pair of HIP events (median / min / max), the
candidates taking turns:

* the fused upsample + CE forward, weighted (rtsds_upce_weighted_fwd) against unweighted
  (rtsds_upce_fwd), at the bench geometry: n = 8, three 19-class heads 64 x 128 -> 512 x 1024, bf16,
  gradients wanted.  Under ``rocprofv3 --kernel-trace --stats`` the two show up as the
  upce_fwd_kernel<..., true> / <..., false> instantiations (the last template argument);
* the label statistics (rtsds_label_stats) on one 8 x 720 x 1280 int64 batch against its traffic
  (8 B per pixel read).

    python tools/bench_wce.py [--out OUT.json] [--reps N]     # default bench_out/wce_time.json
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd._lib import BF16, UPCE_SET_CORRECT, lib  # noqa: E402
from rtsds_amd.runtime import stream  # noqa: E402

DEV = torch.device("cuda", 0)
N, C, HL, WL, K, FACTOR = 8, 19, 64, 128, 3, 8
LS_N, LS_H, LS_W = 8, 720, 1280
ROUNDS = 3


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return {"median_us": round(ts[len(ts) // 2], 2), "min_us": round(ts[0], 2), "max_us": round(ts[-1], 2)}


def upce(reps):
    g = torch.Generator(device=DEV).manual_seed(0)
    heads = [(torch.randn(N, HL, WL, C, device=DEV, generator=g) * 2).bfloat16() for _ in range(K)]
    H, W, s = HL * FACTOR, WL * FACTOR, 1.0 / FACTOR
    t = torch.randint(0, C + 1, (N, H, W), device=DEV, generator=g)        # C = the ignore value
    w = (0.25 + 3.75 * torch.rand(C, device=DEV, generator=g)).float()
    nbytes = lib.rtsds_upce_workspace(K, N, HL, WL, C, H, W, s, s)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    per_head = torch.empty(K, device=DEV)
    total = torch.empty((), device=DEV)
    correct = torch.empty(1, dtype=torch.int64, device=DEV)
    ptrs = (ctypes.c_void_p * K)(*[h.data_ptr() for h in heads])
    flags = 1 | UPCE_SET_CORRECT

    def plain():
        lib.rtsds_upce_fwd(K, ptrs, t.data_ptr(), N, HL, WL, C, H, W, s, s, C, per_head.data_ptr(), total.data_ptr(),
                           correct.data_ptr(), flags, BF16, ws.data_ptr(), nbytes, stream())

    def weighted():
        lib.rtsds_upce_weighted_fwd(K, ptrs, t.data_ptr(), w.data_ptr(), N, HL, WL, C, H, W, s, s, C, per_head.data_ptr(),
                                    total.data_ptr(), correct.data_ptr(), flags, BF16, ws.data_ptr(), nbytes, stream())
    res = {"unweighted": [], "weighted": []}
    for _ in range(ROUNDS):
        res["unweighted"].append(timed(plain, reps))
        res["weighted"].append(timed(weighted, reps))
    return {"geometry": f"n {N}, {K} heads {HL}x{WL} -> {H}x{W}, c {C}, bf16, forward with gradient partials (two launches)", **res}


def label_stats(reps):
    g = torch.Generator(device=DEV).manual_seed(1)
    lab = torch.randint(0, C + 1, (LS_N, LS_H, LS_W), device=DEV, generator=g)
    count = torch.zeros(C, dtype=torch.int64, device=DEV)
    support = torch.zeros_like(count)
    nbytes = lib.rtsds_label_stats_workspace(LS_N, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def run():
        lib.rtsds_label_stats(lab.data_ptr(), LS_N, LS_H, LS_W, C, C, count.data_ptr(), support.data_ptr(), ws.data_ptr(), nbytes,
                              stream())
    # the frequent-class extreme: every pixel one class (the LDS atomics' worst case)
    road = torch.zeros_like(lab)
    res = {"uniform_labels": [timed(run, reps) for _ in range(ROUNDS)]}
    lab.copy_(road)
    res["one_class"] = [timed(run, reps) for _ in range(ROUNDS)]
    nb = LS_N * LS_H * LS_W * 8
    for k in ("uniform_labels", "one_class"):
        med = sorted(r["median_us"] for r in res[k])[ROUNDS // 2]
        res[k + "_GBps"] = round(nb / med / 1e3, 1)
    return {"geometry": f"{LS_N} x {LS_H} x {LS_W} int64, c {C}: {nb} bytes read, two launches", **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("bench_out", "wce_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = {"upce_fwd": upce(a.reps), "label_stats": label_stats(a.reps)}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
