"""Distillation timing (profiles/distill/README.md): functional.distill_kl forward +
backward (rtsds_distill_fwd, rtsds_distill_finish, rtsds_distill_bwd) at the real geometry -- n = 8,
c = 19, the student's 64 x 128 head from the teacher's 65 x 129, T = 1, bf16 and fp32 -- against the
same result from torch ops on the same device: F.interpolate of the teacher, the two scalings,
softmax, log_softmax, kl_div('sum') * T^2 / pixels and their autograd backward.  The two results
are compared before anything is timed.  ROUNDS interleaved repetitions of each; per repetition 5
warm-up calls, then REPS calls each timed by its own pair of HIP events (median / min / max),
forward and backward together.  The bytes each side moves are counted from the shapes.  Both sides
go through autograd, whose host work per call exceeds these kernels' run time, so the three entry
points are also timed as bare ctypes calls on preallocated buffers ("entries").

For information (the teacher's forward dominates): train.seg_step of BiSeNet-R18 against
distill.distill_step with a DeepLabV2-R101 teacher at 1024 x 512, batch 8, bf16, in img/s.

    python tools/bench_distill.py [--out OUT.json] [--no-step]   # default bench_out/distill_time.json
"""
import json
import os
import sys

import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtsds_amd  # noqa: E402
from rtsds_amd import distill, losses, optim, train  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd._lib import lib  # noqa: E402
from rtsds_amd.runtime import stream  # noqa: E402

DEV = torch.device("cuda", 0)
N, C, HS, WS, HT, WT, TEMP = 8, 19, 64, 128, 65, 129, 1.0
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


def torch_chain(s, t):
    u = TF.interpolate(t, size=(HS, WS), mode="bilinear", align_corners=False)
    return TF.kl_div(TF.log_softmax(s / TEMP, 1), TF.softmax(u / TEMP, 1), reduction="sum") * (TEMP * TEMP / (N * HS * WS))


def traffic(esz):
    """Bytes moved, from the shapes.  Fused: the forward reads both heads and writes the fp32
    residual, the backward reads it and writes dx.  torch: every op of the chain reads its inputs
    and writes its output in the storage type (forward: interpolate, two scalings, softmax,
    log_softmax, kl_div's pointwise map and its sum; backward: kl_div, log_softmax, scaling)."""
    se, te = N * HS * WS * C, N * HT * WT * C
    fused = (se + te) * esz + 4 * se + 4 * se + se * esz
    fwd = (te + se) + 2 * se + 2 * se + 2 * se + 2 * se + 3 * se + se   # interp, s/T, u/T, softmax, log_softmax, kl pointwise, sum
    bwd = 3 * se + 3 * se + 2 * se                                      # kl_div, log_softmax, s/T backward
    return {"fused": fused, "torch": (fwd + bwd) * esz}


def kernel_bench(dtype):
    g = torch.Generator(device=DEV).manual_seed(0)
    mk = lambda h, w: (4.0 * torch.randn((N, h, w, C), generator=g, device=DEV)).to(dtype).permute(0, 3, 1, 2)  # noqa: E731
    s, t = mk(HS, WS).requires_grad_(), mk(HT, WT)

    def fused():
        s.grad = None
        F.distill_kl(s, t, TEMP).backward()

    def chain():
        s.grad = None
        torch_chain(s, t).backward()

    nbytes = lib.rtsds_distill_workspace(N, HS, WS, C, HT, WT)
    wsp = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    loss_e, one = torch.empty((), dtype=torch.float32, device=DEV), torch.ones((), dtype=torch.float32, device=DEV)
    dx_e = torch.empty_like(s.detach())
    sh, sw, px, dc = F._src_scale(HT, HS, None), F._src_scale(WT, WS, None), float(N * HS * WS), F.dcode(s)

    def entries():
        lib.rtsds_distill_fwd(s.data_ptr(), dc, t.data_ptr(), dc, N, HS, WS, C, HT, WT, sh, sw, 1.0 / TEMP, 1, None, wsp.data_ptr(),
                              nbytes, stream())
        lib.rtsds_distill_finish(wsp.data_ptr(), nbytes, N, HS, WS, TEMP * TEMP / px, loss_e.data_ptr(), stream())
        lib.rtsds_distill_bwd(wsp.data_ptr(), nbytes, one.data_ptr(), TEMP / px, dx_e.data_ptr(), dc, N, HS, WS, C, stream())

    fused()
    entries()
    torch.cuda.synchronize()
    assert torch.equal(loss_e, F.distill_kl(s, t, TEMP).detach()) and torch.equal(dx_e, s.grad)
    lf, gf = F.distill_kl(s, t, TEMP).detach().double(), s.grad.double().clone()
    chain()
    lt, gt = torch_chain(s, t).detach().double(), s.grad.double().clone()
    s64 = s.detach().double().requires_grad_()
    l64 = torch_chain(s64, t.double())
    l64.backward()
    torch.cuda.synchronize()
    gmax = float(s64.grad.abs().max())
    err = {"fused_loss_rel": abs(float(lf - l64.detach())) / float(l64.detach()),
           "torch_loss_rel": abs(float(lt - l64.detach())) / float(l64.detach()),
           "fused_grad_of_max": float((gf - s64.grad).abs().max()) / gmax, "torch_grad_of_max": float((gt - s64.grad).abs().max()) / gmax}
    lim = 2e-6 if dtype == torch.float32 else 2.0 ** -7      # a bf16 gradient element carries its own rounding
    assert err["fused_loss_rel"] <= 2e-6 and err["fused_grad_of_max"] <= lim, ("the kernels and torch fp64 differ", err)
    assert abs(float(lf - lt)) <= (1e-5 if dtype == torch.float32 else 2e-2) * float(l64.detach()), \
        ("the kernels and the torch chain differ", err)
    res = {"error_against_torch_fp64": err, "bytes": traffic(s.element_size()),
           "fwd_bwd": interleaved({"fused": fused, "torch": chain, "entries": entries})}
    print(str(dtype), json.dumps(res), flush=True)
    return res


def step_bench():
    from oracle.weights import recipe_state_dict, synthetic_images, synthetic_labels
    from rtsds_amd.models.bisenet.build_bisenet import BiSeNet
    from rtsds_amd.models.deeplabv2.deeplabv2 import get_deeplab_v2

    def load(net, seed):
        net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed))
        return net.to(DEV)

    h, w = STEP_SIZE
    x = synthetic_images(STEP_BATCH, h, w, seed=42).to(DEV)
    y = synthetic_labels(STEP_BATCH, h, w, seed=43).to(DEV)
    crit = losses.CrossEntropyLoss(ignore_index=19)
    out = {}
    with rtsds_amd.precision(torch.bfloat16):
        d = distill.Distiller(load(get_deeplab_v2(19, pretrain=False), 3), temperature=TEMP, weight=1.0)
        for name in ("seg_step", "distill_step", "seg_step", "distill_step"):   # taking turns
            net = load(BiSeNet(19, "resnet18"), 1).train()
            opt = optim.Adam(net.parameters(), lr=1e-4)
            step = (lambda: train.seg_step(net, crit, opt, x, y)) if name == "seg_step" else \
                (lambda: distill.distill_step(net, d, crit, opt, x, y))
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
    path = os.path.join("bench_out", "distill_time.json")
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    res = {"geometry": {"n": N, "c": C, "student": [HS, WS], "teacher": [HT, WT], "temperature": TEMP}, "reps": REPS, "rounds": ROUNDS,
           "bf16": kernel_bench(torch.bfloat16), "fp32": kernel_bench(torch.float32)}
    if "--no-step" not in args:
        res["steps_1024x512_bs8_bf16"] = step_bench()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
