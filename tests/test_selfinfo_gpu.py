"""AdvEnt's discriminator input on the device (rtsds_upselfinfo_fwd / _bwd, functional.upsample_self_information)
against the float64 statement of tests/selfinfo_ref.py, with the tolerances pinned in tests/pinned/selfinfo_tol.json
(m * max(E32, 2^-23 M), 2^-8 |ref| per element on top for a bf16 output; tests/test_selfinfo_cpu.py shows that they
reject the wrong kernels).  The cases, and which branch of the host planning each takes, are listed in selfinfo_ref.GEOS.

Every output lies between guard bytes away from a page boundary: y 48 bytes into its allocation (the 16-byte chunks of
the padded rows need that alignment and no more), dx one element past a 16-byte boundary."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd._lib import load  # noqa: E402

from tests import entropy_ref  # noqa: E402
from tests import route_compare as RC  # noqa: E402
from tests import selfinfo_ref as R  # noqa: E402
from tests.bn_bits_cases import BF16, F32  # noqa: E402
from tests.resize_bits_cases import _scale  # noqa: E402

DEV = torch.device("cuda", 0)
PINNED = R.pinned()
GUARD, SENTINEL = 64, 0xA5
ALL = list(range(len(R.CASES)))


def _tdt(dt):
    return torch.bfloat16 if dt == BF16 else torch.float32


class Guarded:
    """``nbytes`` of output between two guards of sentinel bytes, ``offset`` bytes past a 64-byte boundary."""

    def __init__(self, nbytes, offset):
        self.raw = torch.full((nbytes + 2 * GUARD + offset,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.lo, self.hi = GUARD + offset, GUARD + offset + nbytes
        self.ptr = self.raw.data_ptr() + self.lo
        assert self.raw.data_ptr() % 64 == 0

    def host(self, dtype):
        raw = self.raw.cpu()
        assert bool((raw[:self.lo] == SENTINEL).all()) and bool((raw[self.hi:] == SENTINEL).all()), "store outside the output"
        return raw[self.lo:self.hi].clone().view(dtype)


def run_entries(k, x, dy):
    """The raw entries on guarded outputs: x and dy as flat fp32 host arrays.  {"y": [n ho wo y_ld], "dx": [n hi wi c]}
    on the host, in the case's dtype."""
    lib = load()   # the raw entry points: a return code, no exception
    n, hi, wi, c, ho, wo, dt = (k[a] for a in ("n", "hi", "wi", "c", "ho", "wo", "dt"))
    sh, sw, t = _scale(hi, ho), _scale(wi, wo), _tdt(dt)
    esz = 2 if dt == BF16 else 4
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(t)
    dyd = torch.from_numpy(np.ascontiguousarray(dy)).to(DEV).to(t)
    y, dx = Guarded(n * ho * wo * k["yld"] * esz, 48), Guarded(n * hi * wi * c * esz, 16 + esz)
    nws = lib.rtsds_upselfinfo_bwd_workspace(n, hi, wi, c, ho, wo)
    ws = Guarded(nws, 0)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.rtsds_upselfinfo_fwd(xd.data_ptr(), y.ptr, n, hi, wi, c, ho, wo, sh, sw, k["yld"], dt, st) == 0
    assert lib.rtsds_upselfinfo_bwd(dyd.data_ptr(), k["dyld"], xd.data_ptr(), dx.ptr, n, hi, wi, c, ho, wo, sh, sw, dt, ws.ptr, nws, st) == 0
    torch.cuda.synchronize()
    ws.host(torch.uint8)
    return dict(y=y.host(t), dx=dx.host(t))


def run_case(i):
    h, _ = R.case(i)
    return run_entries(R.CASES[i], h["x"], h["dy"])


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("i", ALL, ids=lambda i: R.IDS[i])
def test_forward_and_backward_against_float64(i):
    got, ref, tols = run_case(i), R.case(i)[1], PINNED[R.IDS[i]]
    k = R.CASES[i]
    ratios = {}
    for name in ("y", "dx"):
        g, want = got[name].double(), ref[name].val.double().flatten()
        print(f"{R.IDS[i]} {name}: off by {float((g - want).abs().max()):.3e} at most, max |ref| {float(want.abs().max()):.3e}, tol {tols[name]:.3e}")
        ratios[name] = RC.check(R.IDS[i], name, got[name], ref[name], tols[name])
    print(f"{R.IDS[i]}: worst error / allowance {ratios}")
    pad = got["y"].view(-1, k["yld"])[:, k["c"]:]
    assert not bool(pad.float().any()) and not bool(torch.signbit(pad.float()).any())      # exact zeros behind the classes


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [19, 7])
def test_special_rows(c, dt):
    k = R.special_case(c, dt)
    dy = R.host_inputs(k)["dy"]
    got = run_entries(k, R.special_head(c).reshape(-1), dy)
    dy_seen = torch.from_numpy(dy).to(_tdt(dt)).double().view(4, c)
    want_y, want_dx = R.special_reference(c, dy_seen)
    y, dx = got["y"].double().view(4, 32)[:, :c], got["dx"].double().view(2, 8, c)
    bf = RC.BF16_OUT if dt == BF16 else 0.0
    tol_y = RC.MARGIN * RC.EPS32 * float(want_y.max())           # values below 1, a few fp32 roundings each
    tol_dx = RC.MARGIN * RC.EPS32 * float(want_dx.abs().max()) * (c + 1)
    print(f"c {c} dt {dt}: I off by {float((y - want_y).abs().max()):.3e} (tol {tol_y:.3e}), dx off by "
          f"{float((dx - want_dx[0]).abs().max()):.3e} (tol {tol_dx:.3e}); constant row I {float(y[1, 0])!r}")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    assert bool(((y - want_y).abs() <= tol_y + bf * want_y.abs()).all())
    assert bool(((dx - want_dx[0]).abs() <= tol_dx + bf * want_dx[0].abs()).all())
    assert torch.equal(dx[0], dx[1]) and torch.equal(dx[:, 0::2], dx[:, 1::2])             # the four pixels of a block
    rows = dx[0, 0::2]
    assert not bool(y[0].any()) and not bool(rows[0].any())                                # one logit at 200: p is 1 or 0
    assert not bool(y[2, [1, 4, c - 1]].any()) and not bool(rows[2, [1, 4, c - 1]].any()) and bool(y[2].any())   # classes at -inf
    assert float(y[3, 2]) == float(y[3, 9 % c])                                            # two equal maxima


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_at_the_identity_geometry_the_classes_sum_to_entropy_loss_s_map(dt):
    """Cross-check against the merged kernel (csrc/entropy.hip): sum_k I_k is the normalised entropy h.  Allowance:
    entropy_loss's pinned map tolerance (its c = 19 entropy case, a per-pixel quantity) plus c times this kernel's
    pinned per-element tolerance, plus the c roundings of a bf16 output."""
    i = R.CASES.index(R._case(R.IDENTITY, dt))
    k = R.CASES[i]
    n, c, hh, ww = k["n"], k["c"], k["hi"], k["wi"]
    x = torch.from_numpy(R.case(i)[0]["x"]).view(n, hh, ww, c).to(DEV).to(_tdt(dt)).permute(0, 3, 1, 2)
    hmap = torch.zeros((n, hh, ww), device=DEV)
    F.entropy_loss(x, "entropy", entropy_map=hmap)
    y = F.upsample_self_information(x, F.upsample_geometry(x, size=(hh, ww)))
    total = y.double().sum(1)
    e_tol = entropy_ref.MARGIN * entropy_ref.pinned()[entropy_ref.key((2, 19, 8, 16), "entropy", 2.0, "bf16" if dt == BF16 else "f32")]["map"]
    allow = e_tol + c * PINNED[R.IDS[i]]["y"] + (RC.BF16_OUT * total if dt == BF16 else 0.0)
    err = (total - hmap.double()).abs()
    print(f"identity dt {dt}: sum of I off the entropy map by {float(err.max()):.3e} at most, allowed {float(torch.as_tensor(allow).min()):.3e}")
    assert bool((err <= allow).all())


# ------------------------------------------------------------------ bit stability
STABLE = [0, 1, 9, 17, 19, 21, 23, 31]   # x8 in both dtypes, two forward tiles, the unstaged forward, ragged backward tiles, tw = 32 and 1


@pytest.mark.parametrize("i", STABLE, ids=lambda i: R.IDS[i])
def test_two_runs_give_equal_bits(i):
    a, b = run_case(i), run_case(i)
    assert torch.equal(a["y"].view(torch.uint8), b["y"].view(torch.uint8)) and torch.equal(a["dx"].view(torch.uint8), b["dx"].view(torch.uint8))


# ------------------------------------------------------------------ the autograd function
def _head(i, nchw=False):
    k = R.CASES[i]
    x = torch.from_numpy(R.case(i)[0]["x"]).view(k["n"], k["hi"], k["wi"], k["c"]).to(DEV).to(_tdt(k["dt"])).permute(0, 3, 1, 2)
    return (x.contiguous() if nchw else x).requires_grad_()


def _dy(i):
    k = R.CASES[i]
    return torch.from_numpy(R.case(i)[0]["dy"]).view(k["n"], k["ho"], k["wo"], k["dyld"])[..., :k["c"]].to(DEV).to(_tdt(k["dt"])).permute(0, 3, 1, 2)


@pytest.mark.parametrize("i", [0, 1, 6, 7], ids=lambda i: R.IDS[i])
def test_function_equals_the_entries_in_either_memory_layout(i):
    k = R.CASES[i]
    assert k["yld"] == 32 and k["dyld"] == k["c"]
    raw = run_case(i)
    for nchw in (False, True):
        x = _head(i, nchw)
        y = F.upsample_self_information(x, F.upsample_geometry(x, size=(k["ho"], k["wo"])))
        assert tuple(y.shape) == (k["n"], k["c"], k["ho"], k["wo"]) and y.dtype == x.dtype and y._rt_cpad == 32
        assert F.is_padded_input(y) and F.is_padded_input(F.detach_padded(y))
        y.backward(_dy(i))
        assert torch.equal(y.detach().permute(0, 2, 3, 1).cpu(), raw["y"].view(k["n"], k["ho"], k["wo"], 32)[..., :k["c"]])
        assert x.grad.dtype == x.dtype and torch.equal(x.grad.permute(0, 2, 3, 1).reshape(-1).cpu(), raw["dx"])


@pytest.mark.parametrize("i", [0, 1, 19], ids=lambda i: R.IDS[i])
def test_an_upstream_gradient_of_a_quarter_scales_dx_exactly(i):
    k = R.CASES[i]
    grads = []
    for g in (1.0, 0.25):
        x = _head(i)
        y = F.upsample_self_information(x, F.upsample_geometry(x, size=(k["ho"], k["wo"])))
        y.backward(_dy(i) * g)
        grads.append(x.grad.float())
    assert bool(grads[0].any()) and torch.equal(grads[1] * 4.0, grads[0])     # a power of two: the same bits, shifted


def test_graph_capture_of_forward_and_backward_replays_on_refreshed_inputs():
    i = 3   # odd sizes, bf16
    k = R.CASES[i]
    assert k["dt"] == BF16
    x = _head(i).detach().clone(memory_format=torch.preserve_format).requires_grad_()
    dy = _dy(i).clone(memory_format=torch.preserve_format)
    geo = F.upsample_geometry(x, size=(k["ho"], k["wo"]))
    torch.autograd.grad(F.upsample_self_information(x, geo), x, dy)              # eager (and the first, warming call)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # a straight line on one stream: forward, width pass, height pass
        y = F.upsample_self_information(x, geo)
        dx, = torch.autograd.grad(y, x, dy)
    for salt in (11, 12):
        with torch.no_grad():
            x.copy_(torch.from_numpy(R.pattern(x.numel(), salt)).view(k["n"], k["hi"], k["wi"], k["c"]).permute(0, 3, 1, 2))
            dy.copy_(torch.from_numpy(R.pattern(dy.numel(), salt + 7) / 4).view(k["n"], k["ho"], k["wo"], k["c"]).permute(0, 3, 1, 2))
        graph.replay()
        torch.cuda.synchronize()
        xe = x.detach().clone(memory_format=torch.preserve_format).requires_grad_()
        ye = F.upsample_self_information(xe, geo)
        ye.backward(dy)
        assert torch.equal(y.detach(), ye.detach()) and torch.equal(dx, xe.grad) and bool(dx.any())


def test_refusals():
    x = torch.zeros((1, 19, 4, 4), device=DEV)
    geo = F.upsample_geometry(x, size=(8, 8))
    with pytest.raises(RuntimeError, match="HIP"):
        F.upsample_self_information(x.cpu(), geo)
    with pytest.raises(RuntimeError, match=r"\[2, 32\]"):
        F.upsample_self_information(torch.zeros((1, 33, 4, 4), device=DEV), geo)
    with pytest.raises(RuntimeError, match=r"\[2, 32\]"):
        F.upsample_self_information(torch.zeros((1, 1, 4, 4), device=DEV), geo)
    with pytest.raises(RuntimeError, match="dtype"):
        F.upsample_self_information(x.half(), geo)
