"""Sliding-window timing (profiles/slide/README.md): functional.slide_paint
(rtsds_slide_paint, one launch, no fp32 canvas) against the chain of ops the package had before
it -- per window functional.upsample_softmax_accumulate into a scratch tensor and a slice add
onto a zeroed fp32 canvas, then functional.argmax_channels, a palette gather and the same integer
blend as torch ops -- whose ids and colours are compared with the kernel's for equality before
anything is timed.  Shape: a 1024 x 2048 canvas, 512 x 1024 windows at stride (256, 512) = 9
windows (18 with their mirrored twins), heads 64 x 128 x 19, one frame; fp32 and bf16; alpha 1.0
(the mask alone) and 0.5 (blended over the frame).  ROUNDS interleaved repetitions of each; per
repetition 5 warm-up calls, then REPS calls each timed by its own pair of HIP events (median / min
/ max).  No time is asserted: whether the fused call is below the chain in every repetition is
recorded.  Also recorded: predict.Predictor(stride=) end to end (BiSeNet-R18, 1024 x 2048 frames on
the device, network size 512 x 1024, bf16), with the resizing Predictor beside it.

    python tools/bench_slide.py [--out OUT.json]   # default bench_out/slide_time.json
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtsds_amd  # noqa: E402
from rtsds_amd import predict, validation  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402

DEV = torch.device("cuda", 0)
REPS, ROUNDS = 20, 3
CANVAS, WINDOW, STRIDE, HEAD, C = (1024, 2048), (512, 1024), (256, 512), (64, 128), 19
DTYPES = ((torch.float32, "fp32"), (torch.bfloat16, "bf16"))
ALPHAS = (1.0, 0.5)


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


def torch_chain(x, geo, table, canvas, tmp, pal, a, frame):
    """The unfused form: a zeroed fp32 canvas, per window its probabilities and a slice add, the
    arg-max of the sums, a gathered colour image, the blend."""
    hw, ww = geo[:2]
    canvas.zero_()
    for k, (y0, x0, m) in enumerate(table):
        F.upsample_softmax_accumulate(x[k:k + 1], geo, tmp, flip=bool(m), accumulate=False)
        canvas[:, y0:y0 + hw, x0:x0 + ww] += tmp
    k = F.argmax_channels(canvas.permute(0, 3, 1, 2))
    col = pal[k]
    if a < 256:
        col = ((a * col.int() + (256 - a) * frame.int() + 128) >> 8).to(torch.uint8)
    return k.to(torch.uint8), col


def predictor_fps(stride, calls=5):
    """Frames per second of predict.Predictor, one device frame in, ids and colours out (bf16)."""
    net = BiSeNet(19, "resnet18").to(DEV).eval()
    p = predict.Predictor(net, WINDOW, alpha=0.5, dtype=torch.bfloat16, stride=stride)
    g = torch.Generator(device=DEV).manual_seed(1)
    frames = [torch.randint(0, 256, CANVAS + (3,), generator=g, dtype=torch.uint8, device=DEV)]
    res = []
    for _ in range(ROUNDS):
        for _ in range(2):
            p(frames)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            p(frames)
        torch.cuda.synchronize()
        res.append(round(calls / (time.perf_counter() - t0), 1))
    return res


def main():
    args = sys.argv[1:]
    path = os.path.join("bench_out", "slide_time.json")
    if args[:1] == ["--out"]:
        path = args[1]
    pal = predict.default_palette().to(DEV)
    res = {"reps": REPS, "rounds": ROUNDS, "cases": {}}
    g = torch.Generator().manual_seed(1)
    frame = torch.randint(0, 256, (1,) + CANVAS + (3,), generator=g, dtype=torch.uint8).to(DEV)
    canvas = torch.empty((1,) + CANVAS + (C,), dtype=torch.float32, device=DEV)
    tmp = torch.empty((1,) + WINDOW + (C,), dtype=torch.float32, device=DEV)
    for flip in (False, True):
        table = validation.slide_table(CANVAS, WINDOW, STRIDE, flip)
        x64 = torch.randn(len(table), C, *HEAD, generator=g, dtype=torch.float64) * 3
        for dt, dname in DTYPES:
            x = x64.to(DEV, dt).contiguous(memory_format=torch.channels_last)
            geo = F.upsample_geometry(x, size=WINDOW)
            for alpha in ALPHAS:
                a = int(alpha * 256)
                ids = torch.empty((1,) + CANVAS, dtype=torch.uint8, device=DEV)
                rgb = torch.empty((1,) + CANVAS + (3,), dtype=torch.uint8, device=DEV)

                def fused():
                    F.slide_paint(x, geo, table, CANVAS, 1, palette=pal, alpha=alpha, frame=frame if a < 256 else None, ids=ids,
                                  rgb=rgb)

                def chain():
                    return torch_chain(x, geo, table, canvas, tmp, pal, a, frame)

                fused()
                want_ids, want_rgb = chain()
                torch.cuda.synchronize()
                assert torch.equal(ids, want_ids) and torch.equal(rgb, want_rgb), ("the chain and the kernel differ", dname, alpha)
                assert want_ids.unique().numel() > C // 2  # no constant map
                name = f"{len(table)} windows{' (flip)' if flip else ''} {dname} alpha={alpha}"
                r = {"fused_vs_chain": interleaved({"fused": fused, "chain": chain})}
                r["fused_below_chain_in_every_round"] = all(f["max_us"] < t["min_us"] for f, t in
                                                            zip(r["fused_vs_chain"]["fused"], r["fused_vs_chain"]["chain"]))
                print(name, json.dumps(r), flush=True)
                res["cases"][name] = r
    del canvas, tmp
    with rtsds_amd.precision(torch.bfloat16):
        res["predictor_frames_per_s"] = {"shape": "BiSeNet-R18, one 1024x2048 frame, network 512x1024, bf16, alpha 0.5",
                                         "stride_256x512": predictor_fps(STRIDE), "resized": predictor_fps(None)}
    print("predictor", json.dumps(res["predictor_frames_per_s"]), flush=True)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
