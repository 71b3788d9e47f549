"""Case table and driver of the resize bit pins (tests/test_resize_bits_gpu.py checks them,
tools/record_resize_bits.py records them into tests/pinned/resize_bits.json).

Every case drives the C ABI directly, so each route of rtsds_amd/csrc/resize.hip is reached
without autograd in the way.  Inputs come from the flat element index (no library's random
generator).  Every output lies inside a larger sentinel-filled allocation, and the driver
asserts the sentinels are intact; a pitched output is pinned with its untouched columns.  Each
case also records the entry point's return code.

Sizes are (hi, wi) -> (ho, wo) of the forward resize; the backward cases read dy at (ho, wo)
and write dx at (hi, wi).  V = 8 (bf16) / 4 (fp32) is the 16-byte vector width.  Every case
runs in both dtypes.

The same cases are compared with a float64 statement of each operation: host_inputs builds the inputs
without a device, run_case_outputs hands back what the launch of run_case wrote (same order of
allocations, same sentinel check) and the return code, tests/resize_route_ref.py states what that must be
and tests/test_resize_route_ref_gpu.py compares the two.
"""
import numpy as np
import torch

from .bn_bits_cases import BF16, F32, _dev, _Outputs, _P, _stream, _tdt, pattern

DTS = (BF16, F32)


def _case(kind, n, c, src, dst, **kw):
    return [dict(kind=kind, n=n, c=c, hi=src[0], wi=src[1], ho=dst[0], wo=dst[1], dt=dt, **kw) for dt in DTS]


def _fwd(n, c, src, dst, ld=0, off=0, s=0):
    return _case("fwd", n, c, src, dst, ld=ld, off=off, s=s)


def _bwd(n, c, src, dst, ld=0, off=0):
    return _case("bwd", n, c, src, dst, ld=ld, off=off)


def _usf(n, c, src, dst, yld):
    return _case("usf", n, c, src, dst, yld=yld)


def _usa(n, c, src, dst, flip, acc, pred):
    return _case("usa", n, c, src, dst, flip=flip, acc=acc, pred=pred)


def _usb(n, c, src, dst, dyld, yld):
    return _case("usb", n, c, src, dst, dyld=dyld, yld=yld)


CASES = sum([
    # ---- rtsds_bilinear_fwd, one case per rung of its ladder
    # group_vec (c, y_ld, y_off multiples of V; ho >= 3 hi) into a pitched slice: 17 * 16 / V = 34 / 68
    # column vectors, one slot of the U unroll live; 150 * 16 / V = 300 / 600, grid.x = 1, so slots
    # 1 (and 2 for fp32) are live on some lanes and clamped on the rest
    _fwd(2, 16, (3, 5), (10, 17), ld=24, off=8), _fwd(2, 16, (2, 40), (7, 150), ld=24, off=8),
    # MODE 0 (vector channels, ho < 3 hi): upsample into a pitch, dense downsample, identity
    _fwd(2, 16, (5, 7), (9, 13), ld=24, off=8), _fwd(2, 16, (9, 13), (4, 6)), _fwd(1, 16, (8, 8), (8, 8)),
    # rowgroup (c = 19 off V, dense, wo * c a multiple of V, ho >= hi): 32 * 19 / V = 76 / 152 vectors,
    # nchunk = min(.., max(1, nv / 64)) = 1 / 2; 64 * 19 / V = 152 / 304 vectors, nchunk = 2 / 4; identity
    _fwd(2, 19, (7, 5), (20, 32)), _fwd(2, 19, (7, 5), (20, 64)), _fwd(1, 19, (8, 8), (8, 8)),
    # rows: the same with ho < hi
    _fwd(2, 19, (9, 6), (4, 8)),
    # MODE 1: wo * c = 31 * 19 is no multiple of V; 2 * 432 * 19 * 4 B > 64 KiB of LDS rejects the row kernels
    _fwd(2, 19, (7, 5), (20, 31)), _fwd(1, 19, (2, 432), (3, 440)),
    # MODE 2: c = 67 > 64 off V, into a pitch
    _fwd(2, 67, (5, 7), (9, 13), ld=72, off=3),
    # ---- rtsds_bilinear_fwd_scaled (always group_vec; s = number of channel scales): one and two scales,
    # groups of ~3 rows and of 1-2 rows; a downsample returns RTSDS_ERR_UNSUPPORTED and leaves y untouched
    _fwd(2, 16, (3, 5), (10, 17), ld=24, off=8, s=1), _fwd(2, 16, (3, 5), (10, 17), ld=24, off=8, s=2),
    _fwd(2, 16, (5, 7), (9, 13), s=2), _fwd(2, 16, (9, 13), (4, 6), s=1),
    # ---- rtsds_bilinear_bwd
    # one-pass kernel, 16-byte vectors (c, dy_ld, dy_off multiples of V): x2 gives mw = 9 < 10, G = 4; x4 gives mw = 13, G = 8
    _bwd(2, 16, (4, 5), (8, 10)), _bwd(2, 16, (3, 5), (12, 20)),
    # the same reading a channel slice of a pitched dy
    _bwd(2, 16, (4, 5), (8, 10), ld=24, off=8), _bwd(2, 16, (3, 5), (12, 20), ld=24, off=8),
    # one-pass kernel, single elements (c off V, dy dense), both G
    _bwd(2, 19, (4, 5), (8, 10)), _bwd(2, 19, (3, 5), (12, 20)), _bwd(2, 3, (4, 5), (8, 10)), _bwd(2, 3, (3, 5), (12, 20)),
    # tabulated two-pass route: a pitch that fits neither fused form
    _bwd(2, 19, (4, 5), (8, 10), ld=20), _bwd(2, 16, (3, 5), (12, 20), ld=17),
    # untabulated W kernel (x64: 128 rows of ~133 weights > 48 KiB) with the tabulated H kernel; the transposed
    # shape takes the tabulated W and the untabulated H kernel
    _bwd(1, 3, (2, 128), (2, 8192), ld=4), _bwd(1, 3, (128, 2), (8192, 2), ld=4),
    # non-integer ragged scale (mw ~ 19, G = 8), vector and scalar; a downsample (G = 4)
    _bwd(2, 16, (13, 17), (97, 129)), _bwd(2, 19, (13, 17), (97, 129)),
    _bwd(2, 16, (9, 13), (4, 6)), _bwd(2, 19, (9, 13), (4, 6)),
    # ---- rtsds_upsoftmax_fwd: two tiles per row, the last of 300 - 256 = 44 (45) pixels
    # staged c == 19: y_ld = 32 (bf16: swizzled 16-byte stores; fp32: stage_out), y_ld = 24 (stage_out), y_ld = 19
    # with odd wo (tiles start off 16-byte alignment: stage_out's element loop)
    _usf(2, 19, (3, 40), (5, 300), 32), _usf(2, 19, (3, 40), (5, 300), 24), _usf(2, 19, (3, 40), (5, 301), 19),
    # staged, runtime class count
    _usf(2, 7, (3, 40), (5, 300), 32), _usf(2, 7, (3, 40), (5, 300), 8),
    # unstaged: a 2:1 downsample whose 256-pixel tile reads ~515 columns, 2 * 515 * 19 * 4 B > 48 KiB
    _usf(1, 19, (2, 1024), (1, 512), 32),
    # ---- rtsds_upsoftmax_acc: staged c == 19, odd wo so the tiles' destinations (76-byte rows) start at each
    # of the four 4-byte phases of a 16-byte chunk; flip x accumulate x pred
    *[_usa(2, 19, (3, 40), (5, 301), f, a, p) for f in (0, 1) for a in (0, 1) for p in (0, 1)],
    # staged runtime class count; unstaged (the forward's shape: 78 KiB of taps)
    _usa(2, 7, (3, 40), (5, 301), 1, 1, 1), _usa(1, 19, (2, 1024), (1, 512), 0, 1, 1), _usa(1, 19, (2, 1024), (1, 512), 1, 0, 0),
    # a last tile of one pixel x 3 classes: head + tail only, no float4
    _usa(2, 3, (2, 9), (3, 257), 0, 1, 1), _usa(2, 3, (2, 9), (3, 257), 1, 1, 1),
    # ---- rtsds_upsoftmax_bwd (tabulated H pass unless noted)
    # c == 19 / runtime c; dy dense / pitched; p rows by 16-byte loads (bf16, y_ld = 32) or scalar (fp32; y_ld = 19)
    _usb(2, 19, (3, 40), (5, 300), 19, 32), _usb(2, 19, (3, 40), (5, 300), 24, 32), _usb(2, 19, (3, 40), (5, 301), 19, 19),
    _usb(2, 7, (3, 40), (5, 300), 7, 32), _usb(2, 7, (3, 40), (5, 300), 8, 8),
    # x64: the staged segment of a 64-column tile does not fit, the tiling settles at 8 (bf16) / 4 (fp32) columns
    _usb(1, 19, (2, 40), (3, 2560), 19, 32),
    # untabulated H pass (x64 rows: the H table exceeds 48 KiB)
    _usb(1, 19, (128, 2), (8192, 2), 19, 32),
], [])


def case_id(case):
    return "-".join(f"{k}{v}" if k != "kind" else str(v) for k, v in case.items())


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


def _scale(i, o):
    return float(np.float32(i) / np.float32(o))


def _geo(k):
    return (k["n"], k["hi"], k["wi"], k["c"], k["ho"], k["wo"], _scale(k["hi"], k["ho"]), _scale(k["wi"], k["wo"]))


def _done(out, rc):
    return out, rc


def _in_fwd(k):
    n, hi, wi, c = k["n"], k["hi"], k["wi"], k["c"]
    return dict(x=pattern(n * hi * wi * c, 1), s1=1 + pattern(n * c, 2) / 16 if k["s"] else None,
                s2=1 + pattern(n * c, 3) / 16 if k["s"] == 2 else None)


def _run_fwd(lib, k, h):
    n, hi, wi, c, ho, wo, sh, sw = _geo(k)
    dt, ld = k["dt"], k["ld"] or c
    x = _dev(h["x"], _tdt(dt))
    out = _Outputs()
    y = out.add("y", n * ho * wo * ld, _tdt(dt))
    if k["s"]:
        s1 = _dev(h["s1"], _tdt(dt))
        s2 = _dev(h["s2"], _tdt(dt)) if k["s"] == 2 else None
        rc = lib.rtsds_bilinear_fwd_scaled(_P(x), _P(s1), _P(s2), y, n, hi, wi, c, ho, wo, sh, sw, k["ld"], k["off"], dt,
                                           _stream())
    else:
        rc = lib.rtsds_bilinear_fwd(_P(x), y, n, hi, wi, c, ho, wo, sh, sw, k["ld"], k["off"], dt, _stream())
    return _done(out, rc)


def _ws(nbytes):
    # 0xff bytes: a read of workspace nobody wrote gives NaN, not whatever an earlier case left
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")


def _in_bwd(k):
    return dict(dy=pattern(k["n"] * k["ho"] * k["wo"] * (k["ld"] or k["c"]), 4) / 4)


def _run_bwd(lib, k, h):
    n, hi, wi, c, ho, wo, sh, sw = _geo(k)
    dt, ld = k["dt"], k["ld"] or c
    dy = _dev(h["dy"], _tdt(dt))
    out = _Outputs()
    dx = out.add("dx", n * hi * wi * c, _tdt(dt))
    ws = _ws(lib.rtsds_bilinear_bwd_workspace(n, hi, wi, c, ho, wo))
    rc = lib.rtsds_bilinear_bwd(_P(dy), dx, n, hi, wi, c, ho, wo, sh, sw, k["ld"], k["off"], dt, _P(ws), ws.numel(), _stream())
    return _done(out, rc)


def _in_us(k):
    n, hi, wi, c, ho, wo = k["n"], k["hi"], k["wi"], k["c"], k["ho"], k["wo"]
    return dict(x=pattern(n * hi * wi * c, 1), acc0=(pattern(n * ho * wo * c, 5) + 8) / 16 if k.get("acc") else None)


def _run_usf(lib, k, h):
    n, hi, wi, c, ho, wo, sh, sw = _geo(k)
    dt = k["dt"]
    x = _dev(h["x"], _tdt(dt))
    out = _Outputs()
    y = out.add("y", n * ho * wo * k["yld"], _tdt(dt))
    rc = lib.rtsds_upsoftmax_fwd(_P(x), y, n, hi, wi, c, ho, wo, sh, sw, k["yld"], dt, _stream())
    return _done(out, rc)


def _run_usa(lib, k, h):
    n, hi, wi, c, ho, wo, sh, sw = _geo(k)
    dt = k["dt"]
    x = _dev(h["x"], _tdt(dt))
    out = _Outputs()
    acc = out.add("acc", n * ho * wo * c, torch.float32, h["acc0"])
    pred = out.add("pred", n * ho * wo, torch.int64) if k["pred"] else None
    rc = lib.rtsds_upsoftmax_acc(_P(x), acc, pred, n, hi, wi, c, ho, wo, sh, sw, k["flip"], k["acc"], dt, _stream())
    return _done(out, rc)


def _in_usb(k):
    pix = k["n"] * k["ho"] * k["wo"]
    return dict(dy=pattern(pix * k["dyld"], 4) / 4, p=(pattern(pix * k["yld"], 6) + 8) / 64)  # p probability-sized, [0, 0.25)


def _run_usb(lib, k, h):
    n, hi, wi, c, ho, wo, sh, sw = _geo(k)
    dt, pix = k["dt"], n * ho * wo
    dy = _dev(h["dy"], _tdt(dt))
    p = _dev(h["p"], _tdt(dt))
    out = _Outputs()
    dx = out.add("dx", n * hi * wi * c, _tdt(dt))
    ws = _ws(lib.rtsds_upsoftmax_bwd_workspace(n, hi, wi, c, ho, wo))
    rc = lib.rtsds_upsoftmax_bwd(_P(dy), k["dyld"], _P(p), k["yld"], dx, n, hi, wi, c, ho, wo, sh, sw, dt, _P(ws), ws.numel(),
                                 _stream())
    return _done(out, rc)


_INPUTS = {"fwd": _in_fwd, "bwd": _in_bwd, "usf": _in_us, "usa": _in_us, "usb": _in_usb}
_RUN = {"fwd": _run_fwd, "bwd": _run_bwd, "usf": _run_usf, "usa": _run_usa, "usb": _run_usb}


def host_inputs(case):
    """The host inputs of one case as numpy arrays (fp32 values; a bf16 case rounds them on the way to the
    device), by name.  No device, no library: the references and the tolerance recorder use them too."""
    return _INPUTS[case["kind"]](case)


def _launch(case):
    from rtsds_amd._lib import load
    lib = load()  # the raw entry points: a nonzero return code is recorded, not raised
    h = host_inputs(case)
    return (h,) + _RUN[case["kind"]](lib, case, h)


def run_case(case):
    """{output name: SHA-256 of its bytes, "rc": return code} of one case; asserts the sentinels."""
    _, out, rc = _launch(case)
    d = out.digests()
    d["rc"] = str(rc)
    return d


def run_case_outputs(case):
    """(host inputs, {output name: host tensor}, return code) of one case, the same launches as run_case;
    asserts the sentinels.  tests/resize_route_ref.py states what the outputs must be."""
    h, out, rc = _launch(case)
    return h, out.host(), (rc,)
