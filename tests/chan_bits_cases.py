"""Case table and driver of the channel-vector bit pins (tests/test_chan_bits_gpu.py checks them,
tools/record_chan_bits.py records them into tests/pinned/chan_bits.json).

Every case drives the C ABI directly, so each route of rtsds_amd/csrc/chan.hip is reached
without autograd in the way.  Inputs come from the flat element index (no library's random
generator).  Every output lies inside a larger sentinel-filled allocation, and the driver
asserts the sentinels are intact; a pitched or sliced output is pinned with its untouched
columns.  Each case also records the entry points' return codes.

Logit layouts ("lay"): nhwc is dense (sc = 1, shw = c: the LDS-staged route when c <= 64 and
the output pitch is c); nchw has sc = hw, shw = 1; slice reads c channels at offset 3 of a
24-channel NHWC tensor (shw = 24 > c).  off = 1 moves the inputs one element off their
16-byte alignment.  The staged kernels take tiles of 256 pixels on at most 4096 blocks
(1024 for the cross-entropy partials), the strided ones 256 pixels per block on at most 8192
(1024; 4096 for argmax): the large c = 3 cases are one tile / one pixel group of 44 past that.
The cross-entropy workspace and the losses are pinned as raw 32-bit words: the cases with a target
out of range ("bad") and with every pixel ignored ("none") hold NaN; every other loss is finite.

The same cases are compared with a float64 statement of each operation: host_inputs builds the inputs
without a device, run_case_outputs hands back what the launches of run_case wrote (same order of
allocations and launches, same sentinel check) and the return codes, tests/chan_route_ref.py states what
that must be and tests/test_chan_route_ref_gpu.py compares the two.
"""
import numpy as np
import torch

from .bn_bits_cases import BF16, F32, _dev, _Outputs, _P, _stream, _tdt, pattern

DTS = (BF16, F32)
SLICE_C, SLICE_OFF = 24, 3
IGNORE = 19
CE_RB = 1024  # workspace: [0, RB) partial sums, [RB, 2 RB) partial counts, [2 RB] = C, [2 RB + 1] = S


def _case(kind, dts=DTS, **kw):
    return [dict(kind=kind, dt=dt, **kw) for dt in dts]


def _sm(kind, n, hw, c, lay="nhwc", ld=0, off=0, dts=DTS):
    return _case(kind, dts, n=n, hw=hw, c=c, lay=lay, ld=ld, off=off)


def _smfb(*a, **kw):
    return _sm("smf", *a, **kw) + _sm("smb", *a, **kw)


def _ce(n, hw, c, lay, tgt="idx"):
    return _case("ce", n=n, hw=hw, c=c, lay=lay, tgt=tgt)


def _am(n, hw, c, lay, null=""):
    return _case("am", n=n, hw=hw, c=c, lay=lay, null=null)


CASES = sum([
    # ---- rtsds_softmax_fwd / rtsds_softmax_bwd, staged: two tiles (256 + 44 pixels, rows of 38 / 76 bytes);
    # kStageMaxC; stage_in's element loop; the tile loop's second trip (4096 blocks, 4097 tiles)
    _smfb(2, 150, 19), _smfb(2, 150, 64), _smfb(2, 150, 19, off=1), _smfb(4, 262155, 3, dts=(BF16,)),
    # strided: c past kStageMaxC; a pitched y / dy (padding columns stored as zeros); NCHW; a channel slice;
    # the grid-stride loop's second trip (8192 blocks x 256 threads)
    _smfb(2, 150, 65), _smfb(2, 150, 19, ld=32), _smfb(2, 150, 19, lay="nchw"), _smfb(2, 150, 19, lay="slice"),
    _smfb(4, 524299, 3, lay="nchw", dts=(F32,)),
    # ---- rtsds_ce_fwd / rtsds_ce_bwd / rtsds_ce_finish, both routes: targets over 0..c - 1 and 19 (ignored);
    # one target outside [0, c) that is not ignored (NaN loss); every pixel ignored (0 / 0); the partial kernels'
    # second trip (1024 blocks; finite sums, so a pixel lost or read at a wrong address there moves the digests)
    _ce(2, 150, 19, "nhwc"), _ce(2, 150, 19, "nchw"), _ce(2, 150, 19, "nhwc", "bad"), _ce(2, 150, 19, "nchw", "bad"),
    _ce(2, 150, 19, "nhwc", "none"), _ce(2, 150, 19, "nchw", "none"),
    _ce(4, 65547, 3, "nhwc"), _ce(4, 65547, 3, "nchw"),
    # ---- rtsds_argmax, both routes (rows with a tie, with a NaN first and with NaNs later); each output null
    # in turn; the second trip (4096 blocks on either route)
    *[_am(2, 150, 19, lay, null) for lay in ("nhwc", "nchw") for null in ("", "out", "tgt", "correct")],
    _am(4, 262155, 3, "nhwc"), _am(4, 262155, 3, "nchw"),
    # ---- rtsds_bce_fwd / rtsds_bce_bwd (fp32 only), rtsds_confusion (integers)
    _case("bce", (F32,), n=1), _case("bce", (F32,), n=300), _case("conf", (F32,), total=300, nc=19),
    # ---- the first half of the file
    # rtsds_gap_fwd: vector and scalar channels; hw = 2056 gives 64 slices (the 8-in-flight loop alone),
    # hw = 2088 gives 65 (its tail too)
    *[_case("gapf", n=1, hw=hw, c=c) for hw in (2056, 2088) for c in (64, 19)],
    *[_case("gapb", n=2, hw=150, c=c, acc=acc) for c in (64, 19) for acc in (0, 1)],
    *[_case("csf", n=2, hw=150, c=19, mode=m) for m in (0, 1)],
    *[_case("csb", n=2, hw=150, c=19, mode=m, outs=o) for m in (0, 1) for o in ("dx", "da")],
    _case("csb", n=2, hw=150, c=64, mode=0, outs="da"),
    # rtsds_ffm_head_eval: nine slices of 256 pixels (eight in flight, then one)
    _case("ffm", n=2, hw=2056, c=19),
], [])


def case_id(case):
    return "-".join(f"{k}{v}" if k != "kind" else str(v) for k, v in case.items())


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


def _done(out, *rcs):
    return out, rcs


def _lay(k):
    """(sn, sc, shw, elements of the whole tensor, element offset of the first logit)."""
    n, hw, c = k["n"], k["hw"], k["c"]
    if k["lay"] == "nchw":
        return c * hw, hw, 1, n * hw * c, 0
    if k["lay"] == "slice":
        return hw * SLICE_C, 1, SLICE_C, n * hw * SLICE_C, SLICE_OFF
    return hw * c, 1, c, n * hw * c, k.get("off", 0)


def _at(t, off):
    return t.data_ptr() + off * t.element_size()


def _vals(nel, off, salt, scale=1.0, shift=0.0):
    """Host values of an input of nel elements that starts ``off`` elements into its allocation."""
    return (pattern(nel + off, salt) + shift) * scale


def _in(values, off, dt):
    t = _dev(values, _tdt(dt))
    return t, _at(t, off)


def _out_at(out, name, nel, off, dt):
    """An output of nel elements, pinned whole; the entry point gets the address of element ``off``."""
    p = out.add(name, nel, _tdt(dt))
    return p + off * out.view(name).element_size()


def _in_smf(k):
    _, _, _, nel, off = _lay(k)
    return dict(x=_vals(nel, off, 1))


def _run_smf(lib, k, h):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    sn, sc, shw, nel, off = _lay(k)
    ld = k["ld"] or c
    x, xp = _in(h["x"], off, dt)
    out = _Outputs()
    y = out.add("y", n * hw * ld, _tdt(dt))
    rc = lib.rtsds_softmax_fwd(xp, sn, sc, shw, y, ld, n, hw, c, dt, _stream())
    return _done(out, rc)


def _in_smb(k):
    n, hw, c = k["n"], k["hw"], k["c"]
    ld, io = k["ld"] or c, k["off"]
    return dict(dy=_vals(n * hw * ld, io, 4, 0.25), y=_vals(n * hw * ld, io, 6, 1 / 64, 8))  # y probability-sized, [0, 0.25)


def _run_smb(lib, k, h):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    sn, sc, shw, nel, off = _lay(k)
    ld, io = k["ld"] or c, k["off"]
    dy, dyp = _in(h["dy"], io, dt)
    y, yp = _in(h["y"], io, dt)
    out = _Outputs()
    dx = _out_at(out, "dx", nel, off if k["lay"] == "slice" else 0, dt)
    rc = lib.rtsds_softmax_bwd(dyp, yp, ld, dx, sn, sc, shw, n, hw, c, dt, _stream())
    return _done(out, rc)


def _targets(pix, c, mode="idx"):
    """Classes 0 .. c - 1 and the ignore value from the index; "bad": one target outside [0, c) that is
    not ignored; "none": every pixel ignored."""
    i = np.arange(pix, dtype=np.int64)
    t = (i * 7 + 3) % (c + 1)
    t[t == c] = IGNORE
    if mode == "bad":
        t[pix // 2] = 25
    elif mode == "none":
        t[:] = IGNORE
    return t


def _words(out, name):
    return out.view(name).view(torch.float32)


def _in_ce(k):
    _, _, _, nel, off = _lay(k)
    return dict(x=_vals(nel, off, 1), tgt=_targets(k["n"] * k["hw"], k["c"], k["tgt"]), gl=np.array([2.0], dtype=np.float32))


def _run_ce(lib, k, h):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    sn, sc, shw, nel, off = _lay(k)
    x, xp = _in(h["x"], off, dt)
    tgt = torch.from_numpy(h["tgt"]).cuda()
    nws = lib.rtsds_ce_workspace() // 4
    unread = np.full(nws, -1, dtype=np.int32)  # 0xffffffff: a word nobody wrote reads as NaN
    out = _Outputs()
    ws = out.add("ws", nws, torch.int32, unread)
    loss = out.add("loss", 1, torch.int32)
    rcs = [lib.rtsds_ce_fwd(xp, sn, sc, shw, _P(tgt), loss, n, hw, c, IGNORE, dt, ws, nws * 4, _stream())]
    gl = _dev(h["gl"])
    dx = out.add("dx", nel, _tdt(dt))
    rcs.append(lib.rtsds_ce_bwd(xp, sn, sc, shw, _P(tgt), _P(gl), ws + 2 * CE_RB * 4, dx, n, hw, c, IGNORE, dt, _stream()))
    # the data-parallel finish: C replaced (as if summed over ranks), loss = S / C
    ws2 = out.add("ws_finish", nws, torch.int32, unread)
    out.view("ws_finish").copy_(out.view("ws"))
    _words(out, "ws_finish")[2 * CE_RB] = 123.0
    loss2 = out.add("loss_finish", 1, torch.int32)
    rcs.append(lib.rtsds_ce_finish(ws2, loss2, _stream()))
    return _done(out, *rcs)


def _in_am(k):
    n, hw, c = k["n"], k["hw"], k["c"]
    pix = n * hw
    r = pattern(pix * c, 1).reshape(pix, c)  # [pixel][class]
    if c > 12:
        p = np.arange(pix)
        r[p % 11 == 2, 0] = np.nan                 # a NaN is the first element
        r[np.ix_(p % 11 == 5, (7, 12))] = np.nan   # NaNs after numbers: the first of them wins
        r[np.ix_(p % 11 == 8, (5, 11))] = 9.0      # a tie above every other value
    v = r.reshape(n, hw, c).transpose(0, 2, 1) if k["lay"] == "nchw" else r
    return dict(x=np.ascontiguousarray(v), tgt=None if k["null"] == "tgt" else _targets(pix, c))


def _run_am(lib, k, h):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    sn, sc, shw, nel, off = _lay(k)
    pix = n * hw
    x = _dev(h["x"], _tdt(dt))
    tgt = None if h["tgt"] is None else torch.from_numpy(h["tgt"]).cuda()
    out = _Outputs()
    o = None if k["null"] == "out" else out.add("out", pix, torch.int64)
    cor = None if k["null"] == "correct" else out.add("correct", 1, torch.int64, np.array([5], dtype=np.int64))
    rc = lib.rtsds_argmax(_P(x), sn, sc, shw, o, _P(tgt), cor, n, hw, c, dt, _stream())
    return _done(out, rc)


def _in_bce(k):
    n = k["n"]
    return dict(x=pattern(n, 1), t=(pattern(n, 2) + 8) / 16, gl=np.array([2.0], dtype=np.float32))


def _run_bce(lib, k, h):
    n = k["n"]
    x, t, gl = _dev(h["x"]), _dev(h["t"]), _dev(h["gl"])
    out = _Outputs()
    loss, dx = out.add("loss", 1, torch.float32), out.add("dx", n, torch.float32)
    rcs = [lib.rtsds_bce_fwd(_P(x), _P(t), loss, n, _stream()), lib.rtsds_bce_bwd(_P(x), _P(t), _P(gl), dx, n, _stream())]
    return _done(out, *rcs)


def _in_conf(k):
    total, nc = k["total"], k["nc"]
    i = np.arange(total, dtype=np.int64)
    return dict(label=(i * 7 + 3) % (nc + 4) - 2, pred=(i * 5 + 1) % nc,  # labels -2 .. nc + 1
                hist0=np.arange(nc * nc, dtype=np.int64))


def _run_conf(lib, k, h):
    total, nc = k["total"], k["nc"]
    label = torch.from_numpy(h["label"]).cuda()
    pred = torch.from_numpy(h["pred"]).cuda()
    out = _Outputs()
    hist = out.add("hist", nc * nc, torch.int64, h["hist0"])
    rc = lib.rtsds_confusion(_P(label), _P(pred), hist, total, nc, _stream())
    return _done(out, rc)


def _ws(nbytes):
    # 0xff bytes: a read of workspace nobody wrote gives NaN, not whatever an earlier case left
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")


def _in_gapf(k):
    return dict(x=pattern(k["n"] * k["hw"] * k["c"], 1))


def _run_gapf(lib, k, h):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    x = _dev(h["x"], _tdt(dt))
    out = _Outputs()
    y = out.add("y", n * c, _tdt(dt))
    ws = _ws(lib.rtsds_gap_workspace(n, hw, c))
    rc = lib.rtsds_gap_fwd(_P(x), y, n, hw, c, dt, _P(ws), ws.numel(), _stream())
    return _done(out, rc)


def _in_gapb(k):
    n, hw, c = k["n"], k["hw"], k["c"]
    return dict(dy=pattern(n * c, 4) / 4, dx0=pattern(n * hw * c, 5) / 8 if k["acc"] else None)


def _run_gapb(lib, k, h):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    dy = _dev(h["dy"], _tdt(dt))
    out = _Outputs()
    dx = out.add("dx", n * hw * c, _tdt(dt), h["dx0"])
    rc = lib.rtsds_gap_bwd(_P(dy), dx, n, hw, c, k["acc"], dt, _stream())
    return _done(out, rc)


def _in_cs(k):
    n, hw, c = k["n"], k["hw"], k["c"]
    return dict(dy=pattern(n * hw * c, 4) / 4, x=pattern(n * hw * c, 1), a=(pattern(n * c, 2) + 8) / 16)


def _run_csf(lib, k, h):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    x, a = _dev(h["x"], _tdt(dt)), _dev(h["a"], _tdt(dt))
    out = _Outputs()
    y = out.add("y", n * hw * c, _tdt(dt))
    rc = lib.rtsds_chscale_fwd(_P(x), _P(a), y, n, hw, c, k["mode"], dt, _stream())
    return _done(out, rc)


def _run_csb(lib, k, h):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    dy, x = _dev(h["dy"], _tdt(dt)), _dev(h["x"], _tdt(dt))
    a = _dev(h["a"], _tdt(dt))
    out = _Outputs()
    dx = out.add("dx", n * hw * c, _tdt(dt)) if k["outs"] == "dx" else None
    da = out.add("da", n * c, _tdt(dt)) if k["outs"] == "da" else None
    ws = _ws(lib.rtsds_gap_workspace(n, hw, c))
    rc = lib.rtsds_chscale_bwd(_P(dy), _P(x), _P(a), dx, da, n, hw, c, k["mode"], dt, _P(ws), ws.numel(), _stream())
    return _done(out, rc)


def _in_ffm(k):
    n, hw, c = k["n"], k["hw"], k["c"]
    return dict(f=pattern(n * hw * c, 1) / 4, w=[pattern(c * c, 11 + i) / 16 for i in range(3)],
                b=[pattern(c, 21 + i) / 8 for i in range(3)])


def _run_ffm(lib, k, h):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    f = _dev(h["f"], _tdt(dt))
    w = [_dev(v, _tdt(dt)) for v in h["w"]]
    b = [_dev(v) for v in h["b"]]
    out = _Outputs()
    y = out.add("out", n * hw * c, _tdt(dt))
    ws = _ws(lib.rtsds_ffm_head_eval_workspace(n, hw, c))
    rc = lib.rtsds_ffm_head_eval(_P(f), _P(w[0]), _P(b[0]), _P(w[1]), _P(b[1]), _P(w[2]), _P(b[2]), y, n, hw, c, dt, _P(ws),
                                 ws.numel(), _stream())
    return _done(out, rc)


_RUN = {"smf": _run_smf, "smb": _run_smb, "ce": _run_ce, "am": _run_am, "bce": _run_bce, "conf": _run_conf, "gapf": _run_gapf,
        "gapb": _run_gapb, "csf": _run_csf, "csb": _run_csb, "ffm": _run_ffm}


_INPUTS = {"smf": _in_smf, "smb": _in_smb, "ce": _in_ce, "am": _in_am, "bce": _in_bce, "conf": _in_conf, "gapf": _in_gapf,
           "gapb": _in_gapb, "csf": _in_cs, "csb": _in_cs, "ffm": _in_ffm}


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
    """{output name: SHA-256 of its bytes, "rc": return codes} of one case; asserts the sentinels."""
    _, out, rcs = _launch(case)
    d = out.digests()
    d["rc"] = ",".join(str(rc) for rc in rcs)
    return d


def run_case_outputs(case):
    """(host inputs, {output name: host tensor}, return codes) of one case, the same launches as run_case;
    asserts the sentinels.  tests/chan_route_ref.py states what the outputs must be."""
    h, out, rcs = _launch(case)
    return h, out.host(), rcs
