"""Entropy-minimisation timing (profiles/entropy/README.md): functional.entropy_loss
forward + backward (rtsds_entropy_fwd, rtsds_entropy_finish, rtsds_entropy_bwd) at the real geometry
-- n = 8, c = 19, the 64 x 128 main head, bf16 and fp32, under each penalty (robust with eta 2) --
against the same result from torch ops on the same device: softmax, log_softmax, their product's sum
over the classes, the penalty, the mean, and their autograd backward.  Both results are compared
with torch fp64 before anything is timed.  ROUNDS interleaved repetitions of each; per repetition 5
warm-up calls, then REPS calls each timed by its own pair of HIP events (median / min / max),
forward and backward together.  Both sides go through autograd, whose host work per call exceeds
these kernels' run time, so the three entry points are also timed as bare ctypes calls on
preallocated buffers ("entries").

For information: train.seg_step of BiSeNet-R18 against entmin.entmin_step (a second, main-head-only
forward and backward on a target batch of the same size) at 1024 x 512, batch 8, bf16, in img/s of
the source batch.

    python tools/bench_entropy.py [--out OUT.json] [--no-step]   # default bench_out/entropy_time.json
"""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtsds_amd  # noqa: E402
from rtsds_amd import entmin, losses, optim, train  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd._lib import lib  # noqa: E402
from rtsds_amd.runtime import stream  # noqa: E402

DEV = torch.device("cuda", 0)
N, C, H, W, ETA = 8, 19, 64, 128, 2.0
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


def torch_chain(x, penalty):
    p = torch.softmax(x, 1)
    if penalty == "max_squares":
        return -0.5 * (p * p).sum(1).mean()
    h = -(p * torch.log_softmax(x, 1)).sum(1) / math.log(C)
    return h.mean() if penalty == "entropy" else ((h * h + 1e-8) ** ETA).mean()


def kernel_bench(dtype, penalty):
    g = torch.Generator(device=DEV).manual_seed(0)
    x = (4.0 * torch.randn((N, H, W, C), generator=g, device=DEV)).to(dtype).permute(0, 3, 1, 2).requires_grad_()

    def fused():
        x.grad = None
        F.entropy_loss(x, penalty, ETA)[0].backward()

    def chain():
        x.grad = None
        torch_chain(x, penalty).backward()

    nbytes = lib.rtsds_entropy_workspace(N, H, W, C)
    wsp = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    loss_e, ment_e = torch.empty((), dtype=torch.float32, device=DEV), torch.empty((), dtype=torch.float32, device=DEV)
    one = torch.ones((), dtype=torch.float32, device=DEV)
    dx_e = torch.empty_like(x.detach())
    coef, dc, code = 1.0 / float(N * H * W), F.dcode(x), F.ENTROPY_PENALTIES[penalty]

    def entries():
        lib.rtsds_entropy_fwd(x.data_ptr(), dc, N, H, W, C, code, ETA, 1, None, wsp.data_ptr(), nbytes, stream())
        lib.rtsds_entropy_finish(wsp.data_ptr(), nbytes, N, H, W, coef, loss_e.data_ptr(), ment_e.data_ptr(), stream())
        lib.rtsds_entropy_bwd(wsp.data_ptr(), nbytes, one.data_ptr(), coef, dx_e.data_ptr(), dc, N, H, W, C, stream())

    fused()
    entries()
    torch.cuda.synchronize()
    assert torch.equal(loss_e, F.entropy_loss(x, penalty, ETA)[0].detach()) and torch.equal(dx_e, x.grad)
    lf, gf = F.entropy_loss(x, penalty, ETA)[0].detach().double(), x.grad.double().clone()
    chain()
    lt, gt = torch_chain(x, penalty).detach().double(), x.grad.double().clone()
    x64 = x.detach().double().requires_grad_()
    l64 = torch_chain(x64, penalty)
    l64.backward()
    torch.cuda.synchronize()
    gmax, lref = float(x64.grad.abs().max()), abs(float(l64.detach()))
    err = {"fused_loss_rel": abs(float(lf - l64.detach())) / lref, "torch_loss_rel": abs(float(lt - l64.detach())) / lref,
           "fused_grad_of_max": float((gf - x64.grad).abs().max()) / gmax, "torch_grad_of_max": float((gt - x64.grad).abs().max()) / gmax}
    # fp32: a few roundings, or what torch's own fp32 evaluation of the same formula loses (max_squares' p_j - S
    # cancels where one class holds nearly all the mass); a bf16 gradient element carries its own rounding
    lim = max(2e-6, 2.0 * err["torch_grad_of_max"]) if dtype == torch.float32 else 2.0 ** -7
    assert err["fused_loss_rel"] <= 2e-6 and err["fused_grad_of_max"] <= lim, ("the kernels and torch fp64 differ", err)
    assert abs(float(lf - lt)) <= (1e-5 if dtype == torch.float32 else 2e-2) * lref, ("the kernels and the torch chain differ", err)
    res = {"error_against_torch_fp64": err, "fwd_bwd": interleaved({"fused": fused, "torch": chain, "entries": entries})}
    print(str(dtype), penalty, json.dumps(res), flush=True)
    return res


def step_bench():
    from oracle.weights import recipe_state_dict, synthetic_images, synthetic_labels
    from rtsds_amd.models.bisenet.build_bisenet import BiSeNet

    def load(net, seed):
        net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed))
        return net.to(DEV)

    h, w = STEP_SIZE
    x = synthetic_images(STEP_BATCH, h, w, seed=42).to(DEV)
    y = synthetic_labels(STEP_BATCH, h, w, seed=43).to(DEV)
    xt = synthetic_images(STEP_BATCH, h, w, seed=44).to(DEV)
    crit = losses.CrossEntropyLoss(ignore_index=19)
    em = entmin.EntropyMinimiser("robust", ETA, 0.005)
    out = {}
    with rtsds_amd.precision(torch.bfloat16):
        for name in ("seg_step", "entmin_step", "seg_step", "entmin_step"):   # taking turns
            net = load(BiSeNet(19, "resnet18"), 1).train()
            opt = optim.Adam(net.parameters(), lr=1e-4)
            step = (lambda: train.seg_step(net, crit, opt, x, y)) if name == "seg_step" else \
                (lambda: entmin.entmin_step(net, em, crit, opt, x, y, xt))
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
    print("steps", json.dumps(out), flush=True)
    return out


def main():
    args = sys.argv[1:]
    path = os.path.join("bench_out", "entropy_time.json")
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    res = {"geometry": {"n": N, "c": C, "head": [H, W], "eta": ETA}, "reps": REPS, "rounds": ROUNDS}
    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        res[name] = {penalty: kernel_bench(dtype, penalty) for penalty in F.ENTROPY_PENALTIES}
    if "--no-step" not in args:
        res["steps_1024x512_bs8_bf16"] = step_bench()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
