"""ClassMix timing: functional.class_presence + functional.classmix against
the unfused torch chain (window slices made contiguous, chosen_lut[label], pseudo_select, two
torch.where, ``chosen`` given) on the same tensors in the same run, at the shipped config's shapes:
N = 4, target 512 x 1024, source 720 x 1280, c = 19, bf16 with a pixel pitch of 4.  Three sets of
window origins: x0 a multiple of 8, even, odd.  Per call 5 warm-up rounds, then 30 repetitions each
timed by its own pair of HIP events (median / min / max), then the same 30 back to back under one
pair.  The chain's result is compared with the kernels' for equality before anything is timed.

    python tools/bench_classmix.py [OUT.json]     # default bench_out/classmix_time.json
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtsds_amd import functional as F  # noqa: E402

DEV = torch.device("cuda", 0)
N, H, W, HS, WS, C, IGNORE, REPS = 4, 512, 1024, 720, 1280, 19, 19, 30


def timed(fn, reps=REPS):
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
    # back to back: one event pair around `reps` calls (launch gaps overlap with execution)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1],
            "back_to_back_us": a.elapsed_time(b) * 1e3 / reps}


def padded(n, h, w, g):
    buf = torch.randn((n, h, w, 4), generator=g, device=DEV).to(torch.bfloat16)
    x = buf.permute(0, 3, 1, 2)[:, :3]
    x._rt_cpad = 4
    return x, buf


def main():
    g = torch.Generator(device=DEV).manual_seed(0)
    src, src_buf = padded(N, HS, WS, g)
    tgt, tgt_buf = padded(N, H, W, g)
    slab = torch.randint(0, C + 1, (N, HS, WS), generator=g, device=DEV)
    pred = torch.randint(0, C, (N, H, W), generator=g, device=DEV).to(torch.uint8)
    cbin = torch.randint(0, 1024, (N, H, W), generator=g, device=DEV).to(torch.int16).view(torch.uint16)
    tbin = torch.randint(0, 1024, (C,), generator=g, device=DEV).to(torch.int32)
    perm = torch.stack([torch.randperm(C) for _ in range(N)]).to(torch.int32).to(DEV)
    out, _ = padded(N, H, W, g)
    out_lab = torch.empty((N, H, W), dtype=torch.int64, device=DEV)
    chosen = torch.empty(N, dtype=F._U32, device=DEV)
    res = {"shape": {"n": N, "target": [H, W], "source": [HS, WS], "c": C, "pix_bytes": 8}, "reps": REPS}
    for name, org in (("x0_multiple_of_8", [(101, 64), (3, 8), (208, 256), (0, 0)]),
                      ("x0_even", [(101, 66), (3, 10), (208, 254), (0, 2)]),
                      ("x0_odd", [(101, 77), (3, 9), (208, 255), (0, 1)])):
        origins = torch.tensor(org, dtype=torch.int32, device=DEV)
        present = F.class_presence(slab, (H, W), origins, C)

        def fused():
            p = F.class_presence(slab, (H, W), origins, C)
            F.classmix(src, slab, tgt, pred, cbin, tbin, perm, origins, IGNORE, present=p, out=out,
                       out_labels=out_lab, chosen=chosen)

        def presence_only():
            F.class_presence(slab, (H, W), origins, C)

        def mix_only():
            F.classmix(src, slab, tgt, pred, cbin, tbin, perm, origins, IGNORE, present=present, out=out,
                       out_labels=out_lab, chosen=chosen)

        fused()
        torch.cuda.synchronize()
        ch = chosen.cpu().view(torch.int32).numpy().view(np.uint32)
        lut = torch.zeros((N, C + 1), dtype=torch.bool)
        for i in range(N):
            for k in range(C):
                lut[i, k] = bool((int(ch[i]) >> k) & 1)
        lut = lut.to(DEV)

        def unfused():
            # given `chosen`: window slices, lookup, pseudo_select, two where (labels are in [0, c])
            win = torch.stack([slab[i, y:y + H, x:x + W] for i, (y, x) in enumerate(org)]).contiguous()
            swin = torch.stack([src_buf[i, y:y + H, x:x + W] for i, (y, x) in enumerate(org)]).contiguous()
            m = torch.stack([lut[i][win[i]] for i in range(N)])
            plab = F.pseudo_select(pred, cbin, tbin, IGNORE)
            lab = torch.where(m, win, plab)
            img = torch.where(m[..., None], swin, tgt_buf)
            return lab, img

        lab, img = unfused()
        torch.cuda.synchronize()
        assert torch.equal(lab, out_lab), "unfused labels differ"
        ob = torch.as_strided(out, (N, H, W, 4), (H * W * 4, W * 4, 4, 1))
        assert torch.equal(img.view(torch.int16), ob.view(torch.int16)), "unfused image differs"
        r = {"fused": timed(fused), "presence": timed(presence_only), "classmix": timed(mix_only),
             "unfused": timed(unfused)}
        px = N * H * W
        r["presence_bytes"] = 8 * px
        r["classmix_bytes"] = (8 + 3 + 2 * 8 + 8 + 8) * px
        r["presence_gbs"] = r["presence_bytes"] / r["presence"]["median_us"] / 1e3
        r["classmix_gbs"] = r["classmix_bytes"] / r["classmix"]["median_us"] / 1e3
        res[name] = r
        print(name, json.dumps(r), flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("bench_out", "classmix_time.json")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
