"""Residual BatchNorms with functional.RES_BN_PAIR and RES_BN_BITS on against both off, bit for bit: the mask
bits a residual BatchNorm + ReLU keeps instead of its output (A), the Function that stands for a
residual block's last BatchNorm and its downsample BatchNorm (B) against the two BatchNormFns, the
fallbacks, the residual blocks of both backbones, and BiSeNet-R18 training steps eagerly and as
hipGraph replays."""
import hashlib

import pytest
import torch

import rtsds_amd
from rtsds_amd import functional as F
from rtsds_amd import losses, optim
from rtsds_amd import train as rtrain
from rtsds_amd._lib import ACT_LEAKY, ACT_RELU
from rtsds_amd.models.bisenet import build_contextpath as cp
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet
from rtsds_amd.models.deeplabv2 import deeplabv2 as dl
from rtsds_amd.nn import BatchNorm2d, Conv2d

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
CL = torch.channels_last
DTYPES = [torch.bfloat16, torch.float32]
# rows x c as (n, c, h, w): one row pair; an odd row count on one channel vector; rows and channel
# vectors off every power of two; several rows per thread; several row blocks with a row count that
# is no multiple of the rows in flight; more channel vectors than a block's 256 threads hold rows of
SHAPES = [(2, 8, 1, 1), (1, 8, 5, 7), (1, 24, 37, 1), (3, 64, 10, 10), (1, 128, 41, 100), (1, 2048, 3, 3)]


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


class _Switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):  # (on None: the switches as they are set, the shipped defaults)
        self.was = F.RES_BN_PAIR, F.RES_BN_BITS
        if self.on is not None:
            F.RES_BN_PAIR = F.RES_BN_BITS = self.on

    def __exit__(self, *exc):
        F.RES_BN_PAIR, F.RES_BN_BITS = self.was


def _bn_operands(c, g, arena, zeros=True, beta0=0.5):
    """gamma, beta (leaves), running_mean, running_var, num_batches_tracked of one BatchNorm.  ``zeros``:
    channels 0 and 1 have gamma 0, so their pre-activation is beta + residual exactly (see _residual)."""
    gamma = (torch.randn(c, generator=g) * 0.5 + 1.0)
    beta = torch.randn(c, generator=g) * 0.5
    if zeros:
        gamma[0], beta[0] = 0.0, beta0
        gamma[1], beta[1] = 0.0, -0.0
    gamma = torch.nn.Parameter(gamma.to(DEV))
    beta = torch.nn.Parameter(beta.to(DEV))
    rm = (torch.randn(c, generator=g) * 0.1).to(DEV)
    rv = (torch.rand(c, generator=g) + 0.5).to(DEV)
    nbt = torch.tensor(3, dtype=torch.int64, device=DEV)
    opt = None
    if arena:  # the parameters belong to an rtsds optimizer: the gradients accumulate into its pre-filled buffers
        opt = optim.Adam([gamma, beta], lr=1e-3)
        for a in opt.arenas():
            a.gflat.copy_(torch.randn(a.gflat.shape, generator=g).to(DEV))
    return gamma, beta, rm, rv, nbt, opt


def _residual(shape, dt, g):
    """A residual whose channel 0 is -0.5 on every other row (the sum with beta 0.5 is exactly +0, on the
    other rows positive or negative) and whose channel 1 is -0.0 / a negative value (the sum with beta
    -0.0 is -0 or negative)."""
    res = torch.randn(shape, generator=g)
    flat = res.permute(0, 2, 3, 1).reshape(-1, shape[1])
    flat[0::2, 0] = -0.5
    flat[0::2, 1] = -0.0
    flat[1::2, 1] = -1.0
    res = flat.reshape(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)
    return res.to(DEV, dt).contiguous(memory_format=CL)


def _run_a(on, dt, shape, arena, act=ACT_RELU, training=True):
    n, c, h, w = shape
    with _Switch(on), rtsds_amd.precision(dt):
        g = torch.Generator().manual_seed(5 + c + n * h * w)
        gamma, beta, rm, rv, nbt, opt = _bn_operands(c, g, arena)
        x = (torch.randn(shape, generator=g) * 2 + 1).to(DEV, dt).contiguous(memory_format=CL).requires_grad_()
        res = _residual(shape, dt, g).requires_grad_()
        dy = torch.randn(shape, generator=g).to(DEV, dt).contiguous(memory_format=CL)
        y = F.batch_norm(x, gamma, beta, rm, rv, training, 0.1, 1e-5, act, res, nbt if training else None)
        node = y.grad_fn
        saved = node.saved_tensors
        y.backward(dy)
        torch.cuda.synchronize()
        out = {"y": y.detach(), "rm": rm, "rv": rv, "nbt": nbt, "mean": saved[4].clone(), "invstd": saved[5].clone(),
               "dres": res.grad, "dx": x.grad, "dgamma": gamma.grad.clone(), "dbeta": beta.grad.clone()}
        return out, saved[1].dtype


@pytest.mark.parametrize("arena", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_mask_bits_equal_saved_output(shape, dt, arena):
    """A: apply with a residual, then the backward (g = dres, dx, dgamma, dbeta; fresh and accumulating)."""
    ref, kept0 = _run_a(False, dt, shape, arena)
    got, kept1 = _run_a(True, dt, shape, arena)
    assert kept0 == dt and kept1 == torch.uint8  # the output against the mask bits
    _same(ref, got)
    yr = ref["y"].permute(0, 2, 3, 1).reshape(-1, shape[1]).float()
    assert (yr[0::2, 0] == 0).all() and (yr[:, 1] == 0).all()  # the exact +0 / -0 / negative sums
    assert (ref["dres"].permute(0, 2, 3, 1).reshape(-1, shape[1])[:, 1] == 0).all()
    assert (yr > 0).any() and (yr[:, 2:] == 0).any()


def _run_b(on, dt, shape, arena, act=ACT_RELU, training=True, shape_b=None, far=False, zeros=True):
    n, c, h, w = shape
    with _Switch(on), rtsds_amd.precision(dt):
        g = torch.Generator().manual_seed(11 + c + n * h * w)
        ga, ba, rma, rva, nbta, opta = _bn_operands(c, g, arena, zeros)
        # (channel 0: 0.5 + -0.5 = +0 exactly; channel 1: a sum of two signed zeros)
        gb, bb, rmb, rvb, nbtb, optb = _bn_operands(c, g, arena, zeros, beta0=-0.5)
        xa = (torch.randn(shape, generator=g) * 2 + 1).to(DEV, dt).contiguous(memory_format=CL).requires_grad_()
        xb = _residual(shape_b or shape, dt, g)
        if far:  # very different means of the two BatchNorms
            xb = (xb.float() * 3 + 200).to(dt).contiguous(memory_format=CL)
        xb.requires_grad_()
        dy = torch.randn(shape, generator=g).to(DEV, dt).contiguous(memory_format=CL)
        y = F.batch_norm_pair(xa, (ga, ba, rma, rva, 0.1, 1e-5, nbta if training else None), xb,
                              (gb, bb, rmb, rvb, 0.2, 1e-3, nbtb if training else None), training, act)
        node = y.grad_fn
        name = type(node).__name__
        if name == "BatchNormPairFnBackward":
            stats = node.saved_tensors[-4:]
        else:
            stats = node.saved_tensors[4:6] + node.next_functions[3][0].saved_tensors[4:6]
        stats = [t.clone() for t in stats]
        y.backward(dy)
        torch.cuda.synchronize()
        out = {"y": y.detach(), "rma": rma, "rva": rva, "nbta": nbta, "rmb": rmb, "rvb": rvb, "nbtb": nbtb,
               "mean_a": stats[0], "invstd_a": stats[1], "mean_b": stats[2], "invstd_b": stats[3],
               "dxa": xa.grad, "dxb": xb.grad, "dga": ga.grad.clone(), "dba": ba.grad.clone(), "dgb": gb.grad.clone(),
               "dbb": bb.grad.clone()}
        return out, name


@pytest.mark.parametrize("arena", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_pair_equals_two_batchnorms(shape, dt, arena):
    """B: BatchNormPairFn against BatchNormFn(xb) -> BatchNormFn(xa, residual) on the same conv outputs."""
    ref, f0 = _run_b(False, dt, shape, arena)
    got, f1 = _run_b(True, dt, shape, arena)
    assert f0 == "BatchNormFnBackward" and f1 == "BatchNormPairFnBackward"
    _same(ref, got)
    assert int(ref["nbta"]) == 4 and int(ref["nbtb"]) == 4
    yr = ref["y"].permute(0, 2, 3, 1).reshape(-1, shape[1]).float()
    assert (yr[:, :2] == 0).all() and (yr > 0).any() and (yr[:, 2:] == 0).any()


@pytest.mark.parametrize("dt", DTYPES)
def test_pair_with_distant_means(dt):
    ref, _ = _run_b(False, dt, (3, 64, 10, 10), False, far=True, zeros=False)
    got, f1 = _run_b(True, dt, (3, 64, 10, 10), False, far=True, zeros=False)
    assert f1 == "BatchNormPairFnBackward"
    _same(ref, got)
    assert float(ref["mean_b"].min()) > 100 and float(ref["mean_a"].abs().max()) < 10


@pytest.mark.parametrize("case", ["c20", "eval", "leaky", "shapes"])
def test_fallbacks_run_the_chain(case):
    """Channels off the vector width, running statistics, a LeakyReLU after the residual: the chain
    runs with the switch on, with its results.  Two conv outputs of different shapes (same rows and
    channels): the chain runs and fails as it does with the switch off."""
    kw = {"c20": dict(shape=(2, 20, 4, 8)), "eval": dict(shape=(2, 16, 4, 8), training=False),
          "leaky": dict(shape=(2, 16, 4, 8), act=ACT_LEAKY), "shapes": dict(shape=(2, 16, 4, 8), shape_b=(2, 16, 8, 4))}[case]
    shape = kw.pop("shape")
    if case == "shapes":
        # the chain itself refuses a residual of another shape (autograd checks the gradient it
        # returns for it): the switch changes nothing about that -- the pair does not take it
        for on in (False, True):
            with pytest.raises(RuntimeError, match="BatchNormFnBackward returned an invalid gradient"):
                _run_b(on, torch.bfloat16, shape, False, **kw)
        return
    ref, f0 = _run_b(False, torch.bfloat16, shape, False, **kw)
    got, f1 = _run_b(True, torch.bfloat16, shape, False, **kw)
    assert f0 == f1 == "BatchNormFnBackward"
    _same(ref, got)
    # and the single BatchNorm keeps its output there
    ref, k0 = _run_a(False, torch.bfloat16, shape, False, **kw)
    got, k1 = _run_a(True, torch.bfloat16, shape, False, **kw)
    assert k0 == k1 == torch.bfloat16
    _same(ref, got)


def _block(kind):
    if kind == "basic_down":
        ds = torch.nn.Sequential(Conv2d(16, 32, 1, 2, bias=False), BatchNorm2d(32))
        return cp.BasicBlock(16, 32, 2, ds), (2, 16, 9, 11)
    if kind == "bottleneck_down":
        ds = torch.nn.Sequential(Conv2d(16, 32, 1, 1, bias=False), BatchNorm2d(32))
        return cp.Bottleneck(16, 8, 1, ds), (2, 16, 8, 8)
    if kind == "deeplab_bottleneck_down":
        ds = torch.nn.Sequential(Conv2d(16, 32, 1, 1, bias=False), BatchNorm2d(32))
        return dl.Bottleneck(16, 8, 1, 1, ds), (2, 16, 8, 8)
    return cp.BasicBlock(16, 16), (2, 16, 9, 11)


def _run_block(on, kind, dt):
    with _Switch(on), rtsds_amd.precision(dt):
        torch.manual_seed(3)
        m, shape = _block(kind)
        m = m.to(DEV).train()
        g = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() == 1:
                    p.copy_(torch.randn(p.shape, generator=g).to(DEV) * 0.5 + 1.0)
        x = torch.randn(shape, generator=g).to(DEV, dt).contiguous(memory_format=CL).requires_grad_()
        y = m(x)
        name = type(y.grad_fn).__name__
        dy = torch.randn(y.shape, generator=g).to(DEV, dt).contiguous(memory_format=CL)
        y.backward(dy)
        torch.cuda.synchronize()
        out = {"y": y.detach(), "dx": x.grad}
        for k, p in m.named_parameters():
            if p.grad is not None:
                out["grad." + k] = p.grad.detach().clone()
        for k, b in m.named_buffers():
            out["buf." + k] = b.detach().clone()
        return out, name


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["basic_down", "bottleneck_down", "deeplab_bottleneck_down", "basic_identity"])
def test_residual_blocks(kind, dt):
    ref, f0 = _run_block(False, kind, dt)
    got, f1 = _run_block(True, kind, dt)
    assert f0 == "BatchNormFnBackward"
    assert f1 == ("BatchNormFnBackward" if kind == "basic_identity" else "BatchNormPairFnBackward")
    _same(ref, got)
    assert any(k.startswith("grad.") for k in ref)
    dflt, f2 = _run_block(None, kind, dt)  # and as shipped
    assert f2 == (f1 if F.RES_BN_PAIR else f0)
    _same(ref, dflt)


def _state_hash(net, opt):
    h = hashlib.sha256()  # tools/param_hash.py's hashing
    for _, v in net.state_dict().items():
        h.update(v.detach().float().cpu().numpy().tobytes())
    for a in opt.arenas():
        h.update(a.m.cpu().numpy().tobytes())
        h.update(a.v.cpu().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("mode", ["eager", "graphed"])
def test_bisenet_bit_identical(mode):
    """BiSeNet-R18 training steps at 2x3x64x128 with the switches on, off and as shipped: losses, pixel counts and a
    hash of every parameter, buffer and Adam moment equal -- eagerly, and as hipGraph replays (which
    also equal the eager run)."""
    from rtsds_amd.runtime import GraphedStep
    g = torch.Generator().manual_seed(14)
    x = torch.randn(2, 3, 64, 128, generator=g).to(DEV)
    y = torch.randint(0, 20, (2, 64, 128), generator=g).to(DEV)
    ce = losses.CrossEntropyLoss(ignore_index=19)
    runs = []
    with rtsds_amd.precision(torch.bfloat16):
        for on, graphed in ((False, False), (True, False), (None, False)) + \
                (((False, True), (True, True), (None, True)) if mode == "graphed" else ()):
            with _Switch(on):
                torch.manual_seed(8)
                net = BiSeNet(19, "resnet18").to(DEV).train()
                opt = optim.Adam(net.parameters(), lr=1e-3)
                core = lambda: rtrain.seg_step(net, ce, opt, x, y)  # noqa: E731
                # eager: two steps; graphed: GraphedStep's own eager warm-up step, then one replay
                step = GraphedStep(core, [opt], warmup=1) if graphed else core
                ls = [[float(v) for v in step()] for _ in range(1 if graphed else 2)]
                torch.cuda.synchronize()
                runs.append((ls, _state_hash(net, opt)))
    for ls, hsh in runs[1:]:
        assert ls == runs[0][0][-len(ls):]
        assert hsh == runs[0][1]
    assert all(c > 0 for _, c in runs[0][0])
