"""Painted-frame timing (profiles/paint/README.md): functional.upsample_paint
(rtsds_upsample_paint, one launch) against the unfused chain of ops the package had before it --
functional.interpolate_geometry, functional.argmax_channels, a palette gather and the same integer
blend as torch ops -- whose ids and colours are compared with the kernel's for equality before
anything is timed.  Shapes: the head (1, 19, 64, 128) -> 1024 x 2048 and (8, 19, 64, 128) ->
512 x 1024, fp32 and bf16, alpha 0.5 (blend over the frame) and 1.0 (the mask alone).  ROUNDS
interleaved repetitions of each; per repetition 5 warm-up calls, then REPS calls each timed by its
own pair of HIP events (median / min / max).  The fused call must be below the chain in every
repetition at every shape.  Also recorded, ungated: predict.Predictor end to end (BiSeNet-R18,
1024 x 2048 frames on the device, network size 512 x 1024, bf16) at batch 1 and 8.

Kernel variants: a shared library built from an edited csrc/resize.hip alone (the unit has no
dependency on the others), given as NAME=PATH, has its entry point timed interleaved with the
shipped library's, after its outputs are compared with the shipped library's for equality:

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared variant/resize.hip -o bench_out/libpaint_v.so
    python tools/bench_paint.py [--out OUT.json] [NAME=PATH ...]   # default bench_out/paint_time.json
"""
import ctypes
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtsds_amd  # noqa: E402
from rtsds_amd import _lib, predict  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402
from rtsds_amd.runtime import dcode, stream  # noqa: E402

DEV = torch.device("cuda", 0)
REPS, ROUNDS = 20, 3
SHAPES = (((1, 19, 64, 128), (1024, 2048)), ((8, 19, 64, 128), (512, 1024)))
DTYPES = ((torch.float32, "fp32"), (torch.bfloat16, "bf16"))
ALPHAS = (0.5, 1.0)


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


def torch_chain(x, geo, pal, a, frame):
    """The unfused form: full-resolution logits, an int64 map, a gathered colour image, the blend."""
    k = F.argmax_channels(F.interpolate_geometry(x, geo))
    col = pal[k]
    if a < 256:
        col = ((a * col.int() + (256 - a) * frame.int() + 128) >> 8).to(torch.uint8)
    return k.to(torch.uint8), col


def bytes_per_pixel(c, esz, a):
    """(fused, chain) bytes moved per output pixel, the low-resolution head and the palette left
    out.  Fused: ids and colours written, the frame read for a blend.  Chain: the logits written
    and read again, the int64 map written and read twice (the gather, the uint8 ids), the gathered
    colours and the ids written; a blend goes through eight more element-wise ops on int32 images."""
    blend = a < 256
    fused = 1 + 3 + (3 if blend else 0)
    chain = 2 * c * esz + (8 + 8 + 3) + (8 + 1)
    if blend:  # (read, written) of: col.int(), a *, frame.int(), (256 - a) *, +, + 128, >> 8, uint8
        chain += sum(r + w for r, w in ((3, 12), (12, 12), (3, 12), (12, 12), (24, 12), (12, 12), (12, 12), (12, 3)))
    return fused, chain


def bind(path):
    lib = ctypes.CDLL(path)
    fn = lib.rtsds_upsample_paint
    fn.restype, fn.argtypes = _lib.SIGNATURES["rtsds_upsample_paint"]
    return lib


def entry_point(lib, x, geo, pal, a, frame):
    n, c, hi, wi = x.shape
    ho, wo, sh, sw = geo
    ids = torch.empty((n, ho, wo), dtype=torch.uint8, device=DEV)
    rgb = torch.empty((n, ho, wo, 3), dtype=torch.uint8, device=DEV)

    def call():
        rc = lib.rtsds_upsample_paint(x.data_ptr(), frame.data_ptr(), pal.data_ptr(), None, ids.data_ptr(), rgb.data_ptr(), n,
                                      hi, wi, c, ho, wo, sh, sw, a, dcode(x), stream())
        assert rc == 0, rc

    return call, (ids, rgb)


def predictor_fps(batch, calls=10):
    """Frames per second of predict.Predictor, device frames in, ids and colours out (bf16)."""
    net = BiSeNet(19, "resnet18").to(DEV).eval()
    p = predict.Predictor(net, (512, 1024), alpha=0.5, dtype=torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(batch)
    frames = [torch.randint(0, 256, (1024, 2048, 3), generator=g, dtype=torch.uint8, device=DEV) for _ in range(batch)]
    res = []
    for _ in range(ROUNDS):
        for _ in range(3):
            p(frames)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            p(frames)
        torch.cuda.synchronize()
        res.append(round(batch * calls / (time.perf_counter() - t0), 1))
    return res


def main():
    args = sys.argv[1:]
    path = os.path.join("bench_out", "paint_time.json")
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    variants = dict(a.split("=", 1) for a in args)
    libs = {"shipped": bind(_lib.LIB_PATH)}
    libs.update({name: bind(p) for name, p in variants.items()})
    pal = predict.default_palette().to(DEV)
    res = {"reps": REPS, "rounds": ROUNDS, "cases": {}}
    ok = True
    for (n, c, hi, wi), (ho, wo) in SHAPES:
        g = torch.Generator().manual_seed(n)
        x64 = torch.randn(n, c, hi, wi, generator=g, dtype=torch.float64) * 3
        frame = torch.randint(0, 256, (n, ho, wo, 3), generator=g, dtype=torch.uint8).to(DEV)
        for dt, dname in DTYPES:
            x = x64.to(DEV, dt).contiguous(memory_format=torch.channels_last)
            geo = F.upsample_geometry(x, size=(ho, wo))
            for alpha in ALPHAS:
                a = int(alpha * 256)
                ids = torch.empty((n, ho, wo), dtype=torch.uint8, device=DEV)
                rgb = torch.empty((n, ho, wo, 3), dtype=torch.uint8, device=DEV)

                def fused():
                    F.upsample_paint(x, geo, palette=pal, alpha=alpha, frame=frame, ids=ids, rgb=rgb)

                def chain():
                    return torch_chain(x, geo, pal, a, frame)

                fused()
                want_ids, want_rgb = chain()
                torch.cuda.synchronize()
                assert torch.equal(ids, want_ids) and torch.equal(rgb, want_rgb), ("the chain and the kernel differ", n, dname, alpha)
                assert want_ids.unique().numel() > c // 2  # no constant map
                name = f"{n}x{c}x{hi}x{wi}->{ho}x{wo} {dname} alpha={alpha}"
                fb, cb = bytes_per_pixel(c, x.element_size(), a)
                r = {"bytes_per_pixel": {"fused": fb, "chain": cb}, "fused_vs_chain": interleaved({"fused": fused, "chain": chain})}
                r["fused_below_chain_in_every_round"] = all(f["median_us"] < t["median_us"] for f, t in
                                                            zip(r["fused_vs_chain"]["fused"], r["fused_vs_chain"]["chain"]))
                ok = ok and r["fused_below_chain_in_every_round"]
                fns, outs = {}, {}
                for lname, lib in libs.items():
                    fns[lname], outs[lname] = entry_point(lib, x, geo, pal, a, frame)
                    fns[lname]()
                torch.cuda.synchronize()
                for lname in libs:
                    assert torch.equal(outs[lname][0], ids) and torch.equal(outs[lname][1], rgb), (name, lname)
                r["entry_point"] = interleaved(fns)
                print(name, json.dumps(r), flush=True)
                res["cases"][name] = r
    with rtsds_amd.precision(torch.bfloat16):
        res["predictor_frames_per_s"] = {"shape": "BiSeNet-R18, 1024x2048 frames, network 512x1024, bf16, alpha 0.5",
                                         "batch_1": predictor_fps(1), "batch_8": predictor_fps(8)}
    print("predictor", json.dumps(res["predictor_frames_per_s"]), flush=True)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    assert ok, "the fused call is not below the chain in every repetition at every shape"


if __name__ == "__main__":
    main()
