"""Case table and driver of the BatchNorm bit pins (tests/test_bn_bits_gpu.py checks them,
tools/record_bn_bits.py records them into tests/pinned/bn_bits.json).

Every case drives the C ABI directly, so each planning branch of rtsds_amd/csrc/bn.hip is
reached without autograd in the way.  Inputs come from the flat element index (no library's
random generator); gamma, beta, save_mean, save_invstd and the running statistics are built the
same way and used as given, so a forward and a backward case are independent calls.  Every
output lies inside a larger sentinel-filled allocation, and the driver asserts the sentinels
are intact: a store outside the output fails an assertion in memory the test owns.

Shapes are (rows, c), the smallest that reach each branch (VEC = 16-byte vector width when c is
a multiple of it, else 1; tpr = min(ceil(c / VEC), 256) threads per row, rpi = 256 / tpr rows
per block iteration; need = ceil(rows / rpi); backward row blocks rb = min(need, 512,
ceil(need / 8)); rb == 1 takes the one-launch kernel, whose statistics stay in registers when
rows <= 2 * rpi).

The same cases are compared with a float64 statement of each operation: host_inputs builds the inputs
without a device, run_case_outputs hands back what the launches of run_case wrote (same order of
allocations and launches, same sentinel check), tests/bn_route_ref.py states what that must be and
tests/test_bn_route_ref_gpu.py compares the two.
"""
import hashlib

import numpy as np
import torch

F32, BF16 = 0, 1
NONE, RELU, LEAKY, SIGMOID = 0, 1, 2, 3
SENTINEL, UNWRITTEN = 7.0, -3.0
LEAD, TAIL = 256, 4096  # sentinel elements before / after every output (the view stays 16-byte aligned)
MOMENTUM, EPS = 0.1, 1e-5


def _fwd(rows, c, dt, act, res=False, training=1, nrb=0):
    return dict(kind="fwd", rows=rows, c=c, dt=dt, act=act, res=res, training=training, nrb=nrb)


def _bwd(rows, c, dt, act, y=False, dx=True, dres=False, training=1, acc=0):
    return dict(kind="bwd", rows=rows, c=c, dt=dt, act=act, y=y, dx=dx, dres=dres, training=training, acc=acc)


def _part(rows, c, act, nrb, acc=0):
    return dict(kind="part", rows=rows, c=c, dt=BF16, act=act, nrb=nrb, acc=acc)


CASES = [
    # rows <= 64: forward finalize + apply in one launch; backward one launch, shuffle reduction
    # (tpr = 64), statistics kept in registers for the apply (8 <= 2 * rpi)
    _fwd(8, 512, BF16, RELU), _bwd(8, 512, BF16, RELU),
    # one launch, shuffle reduction, second apply loop (24 > 2 * rpi)
    _fwd(24, 512, BF16, RELU), _bwd(24, 512, BF16, RELU),
    # VEC = 4, tpr = 128: serial LDS reduction inside the one-launch kernel, second apply loop
    _fwd(8, 512, F32, RELU), _bwd(8, 512, F32, RELU),
    # VEC = 8 with tpr = 3 (not a power of two), one launch, registers
    _fwd(40, 24, BF16, RELU), _bwd(40, 24, BF16, RELU),
    # one launch with the mask from y: BatchNorm + sigmoid, residual + LeakyReLU (runtime activation)
    _fwd(8, 512, BF16, SIGMOID), _bwd(8, 512, BF16, SIGMOID, y=True),
    _fwd(8, 512, BF16, LEAKY, res=True), _bwd(8, 512, BF16, LEAKY, y=True, dres=True),
    # VEC = 1, tpr = 19, rb = 2: three launches, serial reduction, row-block-major finalize with a
    # channel tail (19 is not a multiple of 16)
    _fwd(162, 19, BF16, RELU), _bwd(162, 19, BF16, RELU),
    _fwd(162, 19, F32, RELU), _bwd(162, 19, F32, RELU),
    # three launches, shuffle reduction, rb = 8; two-row main loop and one-row tail of the applies
    _fwd(2000, 64, BF16, NONE), _bwd(2000, 64, BF16, NONE),
    _fwd(2000, 64, BF16, RELU), _bwd(2000, 64, BF16, RELU),
    _fwd(2000, 64, BF16, LEAKY), _bwd(2000, 64, BF16, LEAKY),
    # residual + ReLU, dx and dres: the statistics pass stores g as dres, the apply reads g
    _fwd(2000, 64, BF16, RELU, res=True), _bwd(2000, 64, BF16, RELU, y=True, dres=True),
    # mask from y without the stored g; apply with one output
    _bwd(2000, 64, BF16, RELU, y=True), _bwd(2000, 64, BF16, RELU, y=True, dx=False, dres=True),
    # two channel blocks (blockIdx.y = 1), the second with another row width in the bf16 case
    _fwd(27, 2304, BF16, NONE, res=True), _bwd(27, 2304, BF16, NONE, y=True, dres=True),
    _fwd(27, 2048, F32, NONE, res=True), _bwd(27, 2048, F32, NONE, y=True, dres=True),
    # channel-major [c][nrb][2] backward partials (the data-gradient epilogue's), > 1 per thread at 300
    _part(2000, 64, RELU, 5), _part(2000, 64, RELU, 300),
    # forward from [c][nrb][4] epilogue statistics; the one-launch forward from them
    _fwd(2000, 64, BF16, RELU, nrb=5), _fwd(2000, 64, BF16, RELU, nrb=300), _fwd(8, 512, BF16, RELU, nrb=3),
    # eval mode: running statistics, B = C = 0
    _fwd(2000, 64, BF16, RELU, training=0), _bwd(2000, 64, BF16, RELU, training=0),
    _fwd(8, 512, BF16, RELU, training=0), _bwd(8, 512, BF16, RELU, training=0),
    # parameter gradients added to preset dgamma / dbeta
    _bwd(2000, 64, BF16, RELU, acc=1), _bwd(8, 512, BF16, RELU, acc=1), _part(2000, 64, RELU, 5, acc=1),
    # BatchNorm + ReLU + MaxPool2d(3, 2, 1) forward, then the gather backward (pooled gradient source)
    dict(kind="pool", n=1, h=20, w=24, c=16, p=1),
]


def case_id(case):
    return "-".join(f"{k}{v}" if k != "kind" else str(v) for k, v in case.items())


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


# ------------------------------------------------------------------------------- inputs
def pattern(n, salt):
    """n values in [-8, 8) from the flat element index; ``salt`` shifts the sequence per tensor."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(7919 * salt)
    return (((i * np.uint64(2654435761)) % np.uint64(65536)).astype(np.float64) / 4096 - 8).astype(np.float32)


def _tdt(dt):
    return torch.bfloat16 if dt == BF16 else torch.float32


def _dev(values, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(values)).to(dtype).cuda()


class _Outputs:
    """Outputs carved out of sentinel-filled allocations."""

    def __init__(self):
        self.items = {}

    def add(self, name, n, dtype, init=None):
        sent = SENTINEL if dtype.is_floating_point else int(SENTINEL)
        arena = torch.full((LEAD + n + TAIL,), sent, dtype=dtype, device="cuda")
        view = arena[LEAD:LEAD + n]
        if init is None:
            view.fill_(UNWRITTEN if dtype.is_floating_point else 0)
        else:
            view.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype))
        self.items[name] = (arena, view, sent)
        return view.data_ptr()

    def view(self, name):
        return self.items[name][1]

    def host(self):
        """{output name: its elements on the host}, after the sentinel check."""
        torch.cuda.synchronize()
        out = {}
        for name, (arena, view, sent) in self.items.items():
            host = arena.cpu()
            guard = torch.cat([host[:LEAD], host[LEAD + view.numel():]])
            assert torch.equal(guard, torch.full_like(guard, sent)), f"{name}: store outside the output"
            out[name] = host[LEAD:LEAD + view.numel()].contiguous()
        return out

    def digests(self):
        out = {}
        for name, body in self.host().items():
            assert not body.is_floating_point() or torch.isfinite(body.float()).all(), f"{name}: not finite"
            out[name] = hashlib.sha256(body.view(torch.uint8).numpy().tobytes()).hexdigest()
        return out


def _params(c):
    """gamma, beta, save_mean, save_invstd, running_mean, running_var (fp32 [c])."""
    gamma = 1 + pattern(c, 11) / 16
    beta = pattern(c, 12) / 8
    mean = 50 + pattern(c, 13) / 8
    invstd = 0.25 + (pattern(c, 14) + 8) / 32
    rmean = 50 + pattern(c, 15) / 4
    rvar = 1 + (pattern(c, 16) + 8) / 2
    return gamma, beta, mean, invstd, rmean, rvar


def _x(n):
    return 50 + pattern(n, 1)  # large mean: the shifted sums matter


def _y(n, act):
    """A stored output as the activation would have left it (the backward's mask source)."""
    v = pattern(n, 3)
    if act == RELU:
        v = np.maximum(v, 0)
    elif act == SIGMOID:
        v = (v + 8) / 16
    return v


def _ws(lib, rows, c):
    # 0xff bytes: a read of workspace nobody wrote gives NaN, not whatever an earlier case left
    return torch.full((lib.rtsds_bn_workspace(rows, c),), 0xFF, dtype=torch.uint8, device="cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _P(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------- drivers
def _fwd_outputs(out, ny, c, dt, rmean, rvar):
    ptrs = [out.add("y", ny, _tdt(dt)), out.add("save_mean", c, torch.float32), out.add("save_invstd", c, torch.float32),
            out.add("running_mean", c, torch.float32, rmean), out.add("running_var", c, torch.float32, rvar),
            out.add("num_batches_tracked", 1, torch.int64, np.array([5], dtype=np.int64))]
    return ptrs


def _fwd_stats(rows, c, nrb):
    """Synthetic [c][nrb][count, mean, M2, 0] partials, positive counts summing to rows."""
    cnt = np.full(nrb, rows // nrb, dtype=np.float32)
    cnt[:rows % nrb] += 1
    assert cnt.min() > 0 and cnt.sum() == rows
    st = np.zeros((c, nrb, 4), dtype=np.float32)
    st[:, :, 0] = cnt[None, :]
    st[:, :, 1] = 50 + pattern(c * nrb, 21).reshape(c, nrb) / 8
    st[:, :, 2] = cnt[None, :] * (1 + (pattern(c * nrb, 22).reshape(c, nrb) + 8) / 8)
    return st


def _in_fwd(k):
    rows, c = k["rows"], k["c"]
    gamma, beta, _, _, rmean, rvar = _params(c)
    return dict(x=_x(rows * c), res=pattern(rows * c, 2) if k["res"] else None, gamma=gamma, beta=beta, rmean=rmean, rvar=rvar,
                stats=_fwd_stats(rows, c, k["nrb"]) if k["nrb"] else None)


def _opt(v, dtype=torch.float32):
    return None if v is None else _dev(v, dtype)


def _launch_fwd(lib, k, h):
    rows, c, dt = k["rows"], k["c"], k["dt"]
    x = _dev(h["x"], _tdt(dt))
    res = _opt(h["res"], _tdt(dt))
    g, b = _dev(h["gamma"]), _dev(h["beta"])
    stats = _opt(h["stats"])
    out = _Outputs()
    y, sm, si, rm, rv, nbt = _fwd_outputs(out, rows * c, c, dt, h["rmean"], h["rvar"])
    ws = _ws(lib, rows, c)
    lib.rtsds_bn_fwd_ld(_P(x), _P(res), y, c, rows, c, _P(g), _P(b), rm, rv, nbt, sm, si, MOMENTUM, EPS, k["training"],
                        k["act"], _P(stats), k["nrb"], dt, _P(ws), ws.numel(), _stream())
    return out, ()


def _bwd_outputs(out, n, c, dt, dx, dres, acc):
    return (out.add("dx", n, _tdt(dt)) if dx else None, out.add("dres", n, _tdt(dt)) if dres else None,
            out.add("dgamma", c, torch.float32, pattern(c, 31) if acc else None),
            out.add("dbeta", c, torch.float32, pattern(c, 32) if acc else None))


def _in_bwd(k):
    rows, c = k["rows"], k["c"]
    gamma, beta, mean, invstd, _, _ = _params(c)
    h = dict(x=_x(rows * c), dy=pattern(rows * c, 4) / 4, y=_y(rows * c, k["act"]) if k.get("y") else None, gamma=gamma,
             beta=beta, mean=mean, invstd=invstd)
    if k["acc"]:
        h.update(dgamma0=pattern(c, 31), dbeta0=pattern(c, 32))
    if k["kind"] == "part":
        h["part"] = pattern(c * k["nrb"] * 2, 23)  # [c][nrb][sum g, sum g (x - mean)]
    return h


def _launch_bwd(lib, k, h):
    rows, c, dt = k["rows"], k["c"], k["dt"]
    x, dy = _dev(h["x"], _tdt(dt)), _dev(h["dy"], _tdt(dt))
    y = _opt(h["y"], _tdt(dt))
    g, b, sm, si = _dev(h["gamma"]), _dev(h["beta"]), _dev(h["mean"]), _dev(h["invstd"])
    out = _Outputs()
    dx, dres, dg, db = _bwd_outputs(out, rows * c, c, dt, k["dx"], k["dres"], k["acc"])
    ws = _ws(lib, rows, c)
    lib.rtsds_bn_bwd_ld(_P(dy), c, _P(x), _P(y), dx, dres, dg, db, rows, c, _P(g), _P(b), _P(sm), _P(si), k["training"],
                        k["act"], k["acc"], dt, _P(ws), ws.numel(), _stream())
    return out, ()


def _launch_part(lib, k, h):
    rows, c, dt, nrb = k["rows"], k["c"], k["dt"], k["nrb"]
    x, dy = _dev(h["x"], _tdt(dt)), _dev(h["dy"], _tdt(dt))
    g, b, sm, si = _dev(h["gamma"]), _dev(h["beta"]), _dev(h["mean"]), _dev(h["invstd"])
    part = _dev(h["part"])
    out = _Outputs()
    dx, _, dg, db = _bwd_outputs(out, rows * c, c, dt, True, False, k["acc"])
    ws = _ws(lib, rows, c)
    lib.rtsds_bn_bwd_part(_P(dy), _P(x), dx, dg, db, rows, c, _P(g), _P(b), _P(sm), _P(si), 1, k["act"], k["acc"],
                          _P(part), nrb, dt, _P(ws), ws.numel(), _stream())
    return out, ()


def pool_geo(k):
    """(ho, wo, rows, pooled elements) of a pool case."""
    n, h, w, c, p = k["n"], k["h"], k["w"], k["c"], k["p"]
    ho, wo = (h + 2 * p - 3) // 2 + 1, (w + 2 * p - 3) // 2 + 1
    return ho, wo, n * h * w, n * ho * wo * c


def _in_pool(k):
    c = k["c"]
    _, _, rows, npool = pool_geo(k)
    gamma, beta, mean, invstd, rmean, rvar = _params(c)
    return dict(x=_x(rows * c), gamma=gamma, beta=beta, mean=mean, invstd=invstd, rmean=rmean, rvar=rvar,
                dyp=pattern(npool, 4) / 4)


def _launch_pool(lib, k, hin):
    n, h, w, c, p = k["n"], k["h"], k["w"], k["c"], k["p"]
    ho, wo, rows, npool = pool_geo(k)
    x = _dev(hin["x"], torch.bfloat16)
    g, b = _dev(hin["gamma"]), _dev(hin["beta"])
    out = _Outputs()
    y, sm, si, rm, rv, nbt = _fwd_outputs(out, npool, c, BF16, hin["rmean"], hin["rvar"])
    idx = out.add("idx", npool, torch.uint8)
    ws = _ws(lib, rows, c)
    lib.rtsds_bn_relu_maxpool_fwd(_P(x), y, idx, n, h, w, c, ho, wo, p, _P(g), _P(b), rm, rv, nbt, sm, si, MOMENTUM, EPS,
                                  1, None, 0, BF16, _P(ws), ws.numel(), _stream())
    # the backward gathers through the forward's argmax bytes; statistics as given
    dyp = _dev(hin["dyp"], torch.bfloat16)
    smg, sig = _dev(hin["mean"]), _dev(hin["invstd"])
    dx, _, dg, db = _bwd_outputs(out, rows * c, c, BF16, True, False, 0)
    lib.rtsds_bn_relu_maxpool_bwd(_P(dyp), idx, _P(x), dx, dg, db, n, h, w, c, ho, wo, p, _P(g), _P(b), _P(smg), _P(sig),
                                  1, 0, BF16, _P(ws), ws.numel(), _stream())
    return out, ()


_INPUTS = {"fwd": _in_fwd, "bwd": _in_bwd, "part": _in_bwd, "pool": _in_pool}
_LAUNCH = {"fwd": _launch_fwd, "bwd": _launch_bwd, "part": _launch_part, "pool": _launch_pool}


def host_inputs(case):
    """The host inputs of one case as numpy arrays (fp32 values; a bf16 case rounds them on the way to the
    device), by name.  No device, no library: the references and the tolerance recorder use them too."""
    return _INPUTS[case["kind"]](case)


def run_case(case):
    """{output name: SHA-256 of its bytes} of one case; asserts the sentinels around every output."""
    from rtsds_amd._lib import lib
    return _LAUNCH[case["kind"]](lib, case, host_inputs(case))[0].digests()


def run_case_outputs(case):
    """(host inputs, {output name: host tensor}, return codes) of one case, the same launches as run_case;
    asserts the sentinels around every output.  tests/bn_route_ref.py states what the outputs must be."""
    from rtsds_amd._lib import lib
    h = host_inputs(case)
    out, rcs = _LAUNCH[case["kind"]](lib, case, h)
    return h, out.host(), rcs
