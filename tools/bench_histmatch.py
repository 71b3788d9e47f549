"""Histogram-matching timing (profiles/histmatch/README.md): rtsds_hist_u8 +
rtsds_hist_match on one 1052 x 1914 GTA5 frame against the torch-op restatement on the same device
(bincount x 3, cumsum x 6, searchsorted x 3, the blend and a gather, int64 temporaries), whose
result is compared with the kernels' for equality before anything is timed.  ROUNDS interleaved
repetitions of each; per repetition 5 warm-up calls, then REPS calls each timed by its own pair of
HIP events (median / min / max).  The pair must be below the chain in every repetition.

Kernel variants: a shared library built from csrc/histmatch.hip alone with other -D settings
(HM_HIST_AGGREGATE, HM_LUT_KERNEL, HM_HIST_BLOCKS, HM_MATCH_BLOCKS), given as NAME=PATH, has its two
entry points timed on a skewed, a constant and a noise image, interleaved with the shipped
library's, after its results are compared with the shipped library's for equality:

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared -DHM_HIST_AGGREGATE=1 -DHM_LUT_KERNEL=1 \\
        rtsds_amd/csrc/histmatch.hip -o bench_out/libhm_agg_lutk.so
    python tools/bench_histmatch.py [--out OUT.json] [NAME=PATH ...]   # default bench_out/histmatch_time.json
"""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtsds_amd import _lib  # noqa: E402
from rtsds_amd import transforms as T  # noqa: E402
from rtsds_amd.runtime import stream  # noqa: E402

DEV = torch.device("cuda", 0)
H, W, REPS, ROUNDS, A = 1052, 1914, 20, 3, 256


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


def torch_chain(img, hist_ref, a):
    """The matching as torch ops; hist_ref int64 [3, 256]."""
    flat = img.view(-1, 3)
    out = torch.empty_like(img)
    oflat = out.view(-1, 3)
    v = torch.arange(256, device=img.device)
    for ch in range(3):
        x = flat[:, ch].long()
        cs = torch.cumsum(torch.bincount(x, minlength=256), 0)
        cr = torch.cumsum(hist_ref[ch], 0)
        m = torch.searchsorted(cr * cs[-1], cs * cr[-1])  # the first t with Cr[t] * Ns >= Cs[v] * Nr
        lut = ((v * (256 - a) + m * a + 128) >> 8).to(torch.uint8)
        oflat[:, ch] = lut[x]
    return out


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("rtsds_hist_u8", "rtsds_hist_match"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def entry_points(lib, img, hist_ref):
    """(hist(), match(), their outputs) of one library on one image."""
    hist = torch.empty((3, 256), dtype=T._U32, device=DEV)
    out = torch.empty_like(img)
    lut = torch.empty((3, 256), dtype=torch.uint8, device=DEV)

    def hist_fn():
        rc = lib.rtsds_hist_u8(img.data_ptr(), 3, H, W, hist.data_ptr(), stream())
        assert rc == 0, rc

    def match_fn():
        rc = lib.rtsds_hist_match(img.data_ptr(), out.data_ptr(), 3, H, W, hist.data_ptr(), hist_ref.data_ptr(), A,
                                  lut.data_ptr(), stream())
        assert rc == 0, rc

    return hist_fn, match_fn, (hist, out, lut)


def main():
    args = sys.argv[1:]
    path = os.path.join("bench_out", "histmatch_time.json")
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    variants = dict(a.split("=", 1) for a in args)
    g = torch.Generator(device=DEV).manual_seed(0)
    images = {
        "skewed": (255 * torch.rand((H, W, 3), generator=g, device=DEV) ** 2.2).to(torch.uint8),
        "constant": torch.full((H, W, 3), 135, dtype=torch.uint8, device=DEV),
        "noise": torch.randint(0, 256, (H, W, 3), generator=g, device=DEV, dtype=torch.uint8),
    }
    ref_img = (255 * torch.rand((1024, 2048, 3), generator=g, device=DEV) ** 0.5).to(torch.uint8)
    hist_ref = T.image_histogram(ref_img)
    hist_ref64 = hist_ref.view(torch.int32).long()
    res = {"shape": [H, W, 3], "reps": REPS, "rounds": ROUNDS, "strength_q8": A,
           "bytes": {"hist": 3 * H * W, "match": 6 * H * W}}

    # ---- the shipped pair against the torch chain
    img = images["skewed"]
    out = torch.empty_like(img)
    hs = torch.empty((3, 256), dtype=T._U32, device=DEV)

    def fused():
        T.image_histogram(img, out=hs)
        T.histogram_match(img, hs, hist_ref, out=out)

    def chain():
        return torch_chain(img, hist_ref64, A)

    fused()
    want = chain()
    torch.cuda.synchronize()
    assert torch.equal(out, want), "the torch chain and the kernels differ"
    assert not torch.equal(out, img)
    res["pair_vs_torch"] = r = interleaved({"fused": fused, "torch": chain})
    print("pair_vs_torch", json.dumps(r), flush=True)
    res["pair_below_torch_in_every_round"] = all(f["median_us"] < t["median_us"]
                                                 for f, t in zip(r["fused"], r["torch"]))

    # ---- the two entry points, shipped library and variants, per image
    libs = {"shipped": bind(_lib.LIB_PATH)}
    libs.update({name: bind(p) for name, p in variants.items()})
    res["entry_points"] = {}
    for iname, im in images.items():
        fns_h, fns_m, outs = {}, {}, {}
        for lname, lib in libs.items():
            fns_h[lname], fns_m[lname], outs[lname] = entry_points(lib, im, hist_ref)
            fns_h[lname]()
            fns_m[lname]()
        torch.cuda.synchronize()
        for lname in libs:
            for got, ref in zip(outs[lname], outs["shipped"]):
                assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8)), (iname, lname)
        r = {"hist": interleaved(fns_h), "match": interleaved(fns_m)}
        res["entry_points"][iname] = r
        print(iname, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    assert res["pair_below_torch_in_every_round"], "the fused pair is not below the torch chain"


if __name__ == "__main__":
    main()
