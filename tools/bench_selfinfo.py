"""AdvEnt discriminator-input timing (profiles/advent/README.md): rtsds_upselfinfo_fwd / _bwd against the
softmax sibling rtsds_upsoftmax_fwd / _bwd at the benchmark's geometry -- n = 8, c = 19, the 64 x 128 head resized to
512 x 1024, padded to 32 channels, bf16 and fp32 -- as bare ctypes calls on preallocated buffers.  ROUNDS interleaved
repetitions, the old and the new op taking turns; per repetition 5 warm-up calls, then REPS calls each timed by its own
pair of HIP events (median / min / max).  A backward is both of its launches (width pass and height pass).

For information: eager train.da_step of BiSeNet-R18 under the two discriminator inputs, 8 + 8 images at 1024 x 512,
bf16, in img/s of the source batch.

    python tools/bench_selfinfo.py [--out OUT.json] [--no-step]   # default bench_out/selfinfo_time.json
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtsds_amd  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import losses, optim, train  # noqa: E402
from rtsds_amd._lib import lib  # noqa: E402
from rtsds_amd.runtime import stream  # noqa: E402

DEV = torch.device("cuda", 0)
N, C, HI, WI, HO, WO, CP = 8, 19, 64, 128, 512, 1024, 32
REPS, ROUNDS = 20, 3
STEP_SIZE, STEP_BATCH, STEP_WARMUP, STEP_REPS = (512, 1024), 8, 5, 20


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
    return {"median_us": round(ts[len(ts) // 2], 2), "min_us": round(ts[0], 2), "max_us": round(ts[-1], 2)}


def interleaved(fns):
    """{name: [ROUNDS results]}, the candidates taking turns."""
    res = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            res[name].append(timed(fn))
    return res


def _median(rs):
    return sorted(r["median_us"] for r in rs)[len(rs) // 2]


def kernel_bench(dtype):
    g = torch.Generator(device=DEV).manual_seed(0)
    x = (4.0 * torch.randn((N, HI, WI, C), generator=g, device=DEV)).to(dtype)
    dy = torch.randn((N, HO, WO, C), generator=g, device=DEV).to(dtype)
    y_sm, y_si = (torch.empty((N, HO, WO, CP), dtype=dtype, device=DEV) for _ in range(2))
    dx_sm, dx_si = torch.empty_like(x), torch.empty_like(x)
    nws = lib.rtsds_upsoftmax_bwd_workspace(N, HI, WI, C, HO, WO)
    assert nws == lib.rtsds_upselfinfo_bwd_workspace(N, HI, WI, C, HO, WO)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    sh, sw, dc = float(HI) / HO, float(WI) / WO, F.dcode(x)
    P = lambda t: t.data_ptr()  # noqa: E731

    fns = {
        "softmax_fwd": lambda: lib.rtsds_upsoftmax_fwd(P(x), P(y_sm), N, HI, WI, C, HO, WO, sh, sw, CP, dc, stream()),
        "selfinfo_fwd": lambda: lib.rtsds_upselfinfo_fwd(P(x), P(y_si), N, HI, WI, C, HO, WO, sh, sw, CP, dc, stream()),
        "softmax_bwd": lambda: lib.rtsds_upsoftmax_bwd(P(dy), C, P(y_sm), CP, P(dx_sm), N, HI, WI, C, HO, WO, sh, sw, dc, P(ws), nws, stream()),
        "selfinfo_bwd": lambda: lib.rtsds_upselfinfo_bwd(P(dy), C, P(x), P(dx_si), N, HI, WI, C, HO, WO, sh, sw, dc, P(ws), nws, stream()),
    }
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    # what is timed is what the tests check: the sum over the classes is the normalised entropy of the softmax
    p = y_sm[..., :C].double()
    h = -(p * torch.log(p.clamp_min(1e-300))).sum(-1) / torch.log(torch.tensor(float(C), dtype=torch.float64))
    off = float((y_si[..., :C].double().sum(-1) - h).abs().max())
    assert off <= (2e-2 if dtype == torch.bfloat16 else 1e-5), off
    assert bool(torch.isfinite(dx_si.float()).all()) and bool(dx_si.any()) and not bool(y_si[..., C:].any())
    res = {"entropy_cross_check_max_abs": off, "us": interleaved(fns)}
    m = {k: _median(v) for k, v in res["us"].items()}
    res["median_of_medians_us"] = m
    res["fwd_ratio_new_over_old"] = round(m["selfinfo_fwd"] / m["softmax_fwd"], 3)
    res["bwd_ratio_new_over_old"] = round(m["selfinfo_bwd"] / m["softmax_bwd"], 3)
    print(str(dtype), json.dumps(res), flush=True)
    return res


def step_bench():
    from oracle.weights import recipe_state_dict, synthetic_images, synthetic_labels
    from rtsds_amd.models.bisenet.build_bisenet import BiSeNet
    from rtsds_amd.models.domain_shift.adversarial.model import TinyDomainDiscriminator

    def load(net, seed):
        net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed))
        return net.to(DEV).train()

    h, w = STEP_SIZE
    x = synthetic_images(STEP_BATCH, h, w, seed=42).to(DEV)
    y = synthetic_labels(STEP_BATCH, h, w, seed=43).to(DEV)
    xt = synthetic_images(STEP_BATCH, h, w, seed=44).to(DEV)
    ce, bce = losses.CrossEntropyLoss(ignore_index=19), losses.BCEWithLogitsLoss()
    out = {}
    with rtsds_amd.precision(torch.bfloat16):
        for name in ("softmax", "self_information") * ROUNDS:   # taking turns
            net, disc = load(BiSeNet(19, "resnet18"), 1), load(TinyDomainDiscriminator(19), 2)
            opt, dopt = optim.Adam(net.parameters(), lr=1e-4), optim.Adam(disc.parameters(), lr=1e-4, weight_decay=1e-4)

            def step():
                return train.da_step(net, disc, opt, dopt, ce, bce, x, y, xt, 0.001, 1, d_input=name)
            for _ in range(STEP_WARMUP):
                step()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(STEP_REPS):
                step()
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b) / STEP_REPS
            out.setdefault(name, []).append({"ms_per_step": round(ms, 3), "img_per_s": round(STEP_BATCH / ms * 1e3, 1)})
    print("da_step", json.dumps(out), flush=True)
    return out


def main():
    args = sys.argv[1:]
    path = os.path.join("bench_out", "selfinfo_time.json")
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    res = {"geometry": {"n": N, "c": C, "head": [HI, WI], "size": [HO, WO], "y_ld": CP}, "reps": REPS, "rounds": ROUNDS,
           "library": os.path.basename(rtsds_amd._lib.LIB_PATH)}
    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        res[name] = kernel_bench(dtype)
    if "--no-step" not in args:
        res["da_step_1024x512_bs8_bf16"] = step_bench()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
