"""Fourier Domain Adaptation timing (profiles/fda/README.md): rtsds_fda_spectrum +
rtsds_fda_apply on one 720 x 1280 frame at b = 7 (beta = 0.01) and b = 36 (beta = 0.05) against the
published recipe as torch ops on the same device (fft2 of the source, abs / angle, fftshift, the
window of the target's amplitudes -- given, not timed -- swapped in, ifftshift, polar, ifft2, real,
round and clamp to uint8), whose result is compared with the kernels' before anything is timed
(off by at most one grey level at no more than 1e-3 of the pixels: the chain itself is fp32).
ROUNDS interleaved repetitions of each; per repetition 5 warm-up calls, then REPS calls each
timed by its own pair of HIP events (median / min / max).  The pair must be below the chain in
every repetition at b = 7; b = 36 is reported as it is.

Kernel variants: a shared library built from csrc/fda.hip alone with other -D settings
(FDA_G_KERNEL, FDA_SPEC_BLOCKS), given as NAME=PATH, has its entry points timed interleaved with the
shipped library's, after its results are compared with the shipped library's for equality:

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared -DFDA_G_KERNEL=1 \\
        rtsds_amd/csrc/fda.hip -o bench_out/libfda_gkernel.so
    python tools/bench_fda.py [--out OUT.json] [NAME=PATH ...]   # default bench_out/fda_time.json
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
H, W, REPS, ROUNDS, BANDS = 720, 1280, 20, 3, (7, 36)


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


def scene(seed, level, swing, grain):
    """Smooth gradients plus noise (the low band carries real energy), uint8 HWC on the device."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    yy = torch.linspace(-0.5, 0.5, H, device=DEV)[:, None, None]
    xx = torch.linspace(-0.5, 0.5, W, device=DEV)[None, :, None]
    k = torch.rand((2, 1, 1, 3), generator=g, device=DEV) * 2 - 1
    img = torch.tensor(level, device=DEV) + swing * (k[0] * yy + k[1] * xx + 0.5 * torch.sin(6.28 * (yy + 1.3 * xx))) \
        + grain * torch.randn((H, W, 3), generator=g, device=DEV)
    return img.round().clamp(0, 255).to(torch.uint8)


def torch_chain(img, amp_t_shifted, b):
    """The published recipe; amp_t_shifted: fftshift(|fft2(target)|), fp32 [3, H, W]."""
    f = torch.fft.fft2(img.permute(2, 0, 1).float())
    amp, pha = torch.fft.fftshift(f.abs(), dim=(-2, -1)), f.angle()
    ys, xs = slice(H // 2 - b, H // 2 + b + 1), slice(W // 2 - b, W // 2 + b + 1)
    amp[:, ys, xs] = amp_t_shifted[:, ys, xs]
    out = torch.fft.ifft2(torch.polar(torch.fft.ifftshift(amp, dim=(-2, -1)), pha)).real
    return out.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("rtsds_fda_workspace", "rtsds_fda_spectrum", "rtsds_fda_apply"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def entry_points(lib, img, amp_t, b):
    """(spectrum(), apply(), their outputs) of one library."""
    spec = torch.empty((3, 2 * b + 1, b + 1, 2), dtype=torch.float32, device=DEV)
    amp = torch.empty((3, 2 * b + 1, b + 1), dtype=torch.float32, device=DEV)
    out = torch.empty_like(img)
    ws = torch.empty(lib.rtsds_fda_workspace(H, W, b), dtype=torch.uint8, device=DEV)

    def spectrum_fn():
        rc = lib.rtsds_fda_spectrum(img.data_ptr(), 3, H, W, b, spec.data_ptr(), amp.data_ptr(), ws.data_ptr(), ws.numel(),
                                    stream())
        assert rc == 0, rc

    def apply_fn():
        rc = lib.rtsds_fda_apply(img.data_ptr(), out.data_ptr(), 1, 3, H, W, b, spec.data_ptr(), amp_t.data_ptr(), 1.0, stream())
        assert rc == 0, rc

    return spectrum_fn, apply_fn, (spec, amp, out)


def main():
    args = sys.argv[1:]
    path = os.path.join("bench_out", "fda_time.json")
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    variants = dict(a.split("=", 1) for a in args)
    src = scene(0, (70.0, 80.0, 100.0), 30.0, 12.0)
    tgt = scene(1, (175.0, 160.0, 140.0), 18.0, 8.0)
    amp_t_shifted = torch.fft.fftshift(torch.fft.fft2(tgt.permute(2, 0, 1).float()).abs(), dim=(-2, -1))
    libs = {"shipped": bind(_lib.LIB_PATH)}
    libs.update({name: bind(p) for name, p in variants.items()})
    res = {"shape": [H, W, 3], "reps": REPS, "rounds": ROUNDS, "strength": 1.0,
           "bytes": {"spectrum": 3 * H * W, "apply": 6 * H * W}, "bands": {}}
    for b in BANDS:
        _, amp_t = T.band_spectrum(tgt, b)
        spec = torch.empty((3, 2 * b + 1, b + 1, 2), dtype=torch.float32, device=DEV)
        amp = torch.empty((3, 2 * b + 1, b + 1), dtype=torch.float32, device=DEV)
        out = torch.empty_like(src)

        def fused():
            T.band_spectrum(src, b, spec=spec, amp=amp)
            T.fourier_adapt(src, spec, amp_t, out=out)

        def chain():
            return torch_chain(src, amp_t_shifted, b)

        fused()
        want = chain()
        torch.cuda.synchronize()
        diff = (out.int() - want.int()).abs()
        moved = (out.int() - src.int()).abs().float().mean().item()
        off = (diff > 0).float().mean().item()
        assert int(diff.max()) <= 1 and off <= 1e-3, ("the torch chain and the kernels differ", b, int(diff.max()), off)
        assert moved >= 5.0, moved
        r = {"flops": {"spectrum": 2 * 2 * 3 * H * W * (b + 1), "apply": 2 * 2 * 3 * H * W * (b + 1)},
             "mean_abs_change": round(moved, 2), "share_off_by_one_vs_torch": off,
             "pair_vs_torch": interleaved({"fused": fused, "torch": chain})}
        print(f"b={b} pair_vs_torch", json.dumps(r["pair_vs_torch"]), flush=True)
        r["pair_below_torch_in_every_round"] = all(f["median_us"] < t["median_us"] for f, t in
                                                   zip(r["pair_vs_torch"]["fused"], r["pair_vs_torch"]["torch"]))
        # ---- the two entry points, shipped library and variants
        fns_s, fns_a, outs = {}, {}, {}
        for lname, lib in libs.items():
            fns_s[lname], fns_a[lname], outs[lname] = entry_points(lib, src, amp_t, b)
            fns_s[lname]()
            fns_a[lname]()
        torch.cuda.synchronize()
        for lname in libs:
            for got, ref in zip(outs[lname], outs["shipped"]):
                assert torch.equal(got, ref), (b, lname)
        assert torch.equal(outs["shipped"][2], out)
        r["entry_points"] = {"spectrum": interleaved(fns_s), "apply": interleaved(fns_a)}
        print(f"b={b} entry_points", json.dumps(r["entry_points"]), flush=True)
        res["bands"][str(b)] = r
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    assert res["bands"]["7"]["pair_below_torch_in_every_round"], "the fused pair is not below the torch chain at b = 7"


if __name__ == "__main__":
    main()
