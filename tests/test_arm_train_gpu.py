"""Training-mode attention refinement chains with AttentionRefinementModule.fused_train on against
the op-by-op chain (switch off), bit for bit: the 16-byte channel-scale kernels against the scalar
ones, the one-pass scale backward against its two passes, ARM1's form (own pool) and ARM2's (given
pool, scaled by the tail, both joins) at op level, the fallback shapes, and BiSeNet-R18 training
steps eagerly, with the main head only, and as hipGraph replays."""
import hashlib

import pytest
import torch

import rtsds_amd
from rtsds_amd import functional as F
from rtsds_amd import losses, optim
from rtsds_amd import train as rtrain
from rtsds_amd._lib import load
from rtsds_amd.models.bisenet.build_bisenet import AttentionRefinementModule, BiSeNet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
CL = torch.channels_last
DTYPES = [torch.bfloat16, torch.float32]


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def _arm_run(fused, form, dt, n, c, h, w, arena, train=True):
    """One forward / backward of an AttentionRefinementModule with non-trivial parameters, as
    BiSeNet._heads runs ARM1 (``form`` 1: own pool) or ARM2 (``form`` 2: the pool given, the result
    scaled by it, f4's and the tail's gradient joins).  ``arena``: the parameters belong to an
    rtsds optimizer, so the weight gradients accumulate into its pre-filled gradient buffers.
    Returns every output, saved tensor, buffer and gradient, and the Functions that ran."""
    AttentionRefinementModule.fused_train = fused
    try:
        with rtsds_amd.precision(dt):
            torch.manual_seed(41)
            m = AttentionRefinementModule(c, c).to(DEV).train(train)
            g = torch.Generator().manual_seed(42)
            with torch.no_grad():
                for p in m.parameters():
                    if p.dim() == 1:  # conv bias, BatchNorm weight / bias
                        p.copy_(torch.randn(p.shape, generator=g).to(DEV) * 0.5 + (1.0 if p is m.bn.weight else 0.0))
                m.bn.running_mean.copy_(torch.randn(c, generator=g).to(DEV) * 0.1)
            if arena:
                opt = optim.Adam(m.parameters(), lr=1e-3)
                for a in opt.arenas():
                    a.gflat.copy_(torch.randn(a.gflat.shape, generator=g).to(DEV))
            x = torch.randn(n, c, h, w, generator=g).to(DEV, dt).contiguous(memory_format=CL).requires_grad_()
            gy = torch.randn(n, c, h, w, generator=g).to(DEV, dt).contiguous(memory_format=CL)
            out = {}
            if form == 1:
                y = m(x)
            else:
                j4 = F.GradJoin(2)
                jt = F.GradJoin(0, first_returns=True)
                tail = F.global_avg_pool(x, j4)
                tail.retain_grad()
                y = m.forward_scaled(x, tail, pooled=tail, join=j4, pooled_join=jt, scale_join=jt)
            fns, node = [], y.grad_fn
            scale = node
            while type(node).__name__.startswith("ChScale"):
                fns.append(type(node).__name__)
                scale = node
                node = node.next_functions[0][0]
            att = scale.saved_tensors[1]  # the attention, as the (inner) scale saved it
            out["att"] = att.detach().clone()
            bn_node = scale.next_functions[1][0]
            if type(bn_node).__name__.startswith("BatchNorm"):  # conv output (the backward's x), save stats
                for i, t in enumerate(bn_node.saved_tensors):
                    out[f"bn_saved{i}"] = t.detach().clone()
            y.backward(gy)
            torch.cuda.synchronize()
            out.update({"y": y.detach(), "dx": x.grad})
            if form == 2:
                out["dtail"] = tail.grad
            for k, p in m.named_parameters():
                out["grad." + k] = p.grad.detach().clone()
            for k, b in m.named_buffers():
                out["buf." + k] = b.detach().clone()
            return out, fns
    finally:
        AttentionRefinementModule.fused_train = True


# 1x8x4x8: one slice, C below a wave's 64 x V channels; 2x64x8x16: several slices; 3x72x5x7: hw off
# the row group, C no multiple of 64; 8x256x4x8: N at the pooled kernels' limit (BiSeNet's ARM1 width)
@pytest.mark.parametrize("arena", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geo", [(1, 8, 4, 8), (2, 64, 8, 16), (3, 72, 5, 7), (8, 256, 4, 8)])
def test_arm1_equals_chain(geo, dt, arena):
    train = True
    if geo[0] == 1:
        # batch statistics over one pooled row: the BatchNorm raises, as torch's does, with either
        # switch; the shape's kernels (the scale and its one-pass backward) run with running statistics
        for fused in (False, True):
            with pytest.raises(ValueError, match="more than 1 value per channel"):
                _arm_run(fused, 1, dt, *geo, arena)
        train = False
    ref, f0 = _arm_run(False, 1, dt, *geo, arena, train=train)
    got, f1 = _arm_run(True, 1, dt, *geo, arena, train=train)
    assert f0 == f1 == ["ChScaleFnBackward"]
    _same(ref, got)
    assert ("bn_saved0" in ref or not train) and "buf.bn.num_batches_tracked" in ref


# 8x1024x2x4: two trips of the pooled GEMV's channel loop, four channel vectors per thread row
@pytest.mark.parametrize("arena", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geo", [(2, 64, 4, 8), (8, 1024, 2, 4)])
def test_arm2_equals_chain(geo, dt, arena):
    ref, f0 = _arm_run(False, 2, dt, *geo, arena)
    got, f1 = _arm_run(True, 2, dt, *geo, arena)
    assert f0 == ["ChScaleFnBackward", "ChScaleFnBackward"] and f1 == ["ChScale2FnBackward"]
    _same(ref, got)
    assert "dtail" in ref and "bn_saved0" in ref


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("geo,train", [((2, 20, 4, 8), True), ((9, 64, 4, 8), True), ((2, 64, 4, 8), False)])
def test_arm_fallback(geo, train, form):
    """C off the vector width, N past the pooled kernels' limit, eval mode (running statistics):
    the chain's results with the switch on, and nothing raises."""
    ref, _ = _arm_run(False, form, torch.bfloat16, *geo, False, train=train)
    got, fns = _arm_run(True, form, torch.bfloat16, *geo, False, train=train)
    if geo[1] % 8:
        assert fns == ["ChScaleFnBackward"] * form
    _same(ref, got)


def _unaligned(t):
    """A copy of ``t`` one element off 16-byte alignment: the library's scalar kernels take it."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16
    return v


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", [8, 24])
def test_vector_scale_kernels_equal_scalar(c, dt, mode):
    """rtsds_chscale_fwd and rtsds_chscale_bwd (dx alone, da alone, and both in one pixel pass) on
    aligned tensors -- the 16-byte kernels -- against the same calls on unaligned copies, which
    run the scalar kernels; an odd pixel count, 3 images."""
    lib = load()
    n, hw = 3, 5 * 7
    code = 1 if dt == torch.bfloat16 else 0
    g = torch.Generator().manual_seed(7 + c + mode)
    x, dy = (torch.randn(n * hw * c, generator=g).to(DEV, dt) for _ in range(2))
    a = torch.randn(n * c, generator=g).to(DEV, dt)
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(lib.rtsds_gap_workspace(n, hw, c), dtype=torch.uint8, device=DEV)
    res = []
    for al in (True, False):
        # (the attention gradient's reduction reads 16-byte vectors whenever c allows: its inputs
        # stay aligned; an unaligned dx alone sends the joint call down the separate passes)
        xi, dyi, ai = (t if al else _unaligned(t) for t in (x, dy, a))
        y, dx, dx2 = ((torch.empty_like(x) if al else _unaligned(x)) for _ in range(3))
        da, da2 = torch.empty_like(a), torch.empty_like(a)
        assert lib.rtsds_chscale_fwd(xi.data_ptr(), ai.data_ptr(), y.data_ptr(), n, hw, c, mode, code, st) == 0
        assert lib.rtsds_chscale_bwd(dyi.data_ptr(), xi.data_ptr(), ai.data_ptr(), dx.data_ptr(), None, n, hw, c, mode, code,
                                     ws.data_ptr(), ws.numel(), st) == 0
        assert lib.rtsds_chscale_bwd(dy.data_ptr(), x.data_ptr(), a.data_ptr(), None, da.data_ptr(), n, hw, c, mode, code,
                                     ws.data_ptr(), ws.numel(), st) == 0
        assert lib.rtsds_chscale_bwd(dy.data_ptr(), x.data_ptr(), a.data_ptr(), dx2.data_ptr(), da2.data_ptr(), n, hw, c, mode,
                                     code, ws.data_ptr(), ws.numel(), st) == 0
        torch.cuda.synchronize()
        res.append({"y": y.clone(), "dx": dx.clone(), "da": da, "dx2": dx2.clone(), "da2": da2})
    _same(res[0], res[1])
    assert torch.equal(res[0]["dx"], res[0]["dx2"]) and torch.equal(res[0]["da"], res[0]["da2"])
    # and the forward against the expression itself (mode 0: one rounding of the exact product)
    if mode == 0:
        ref = (x.view(n, hw, c).float() * a.view(n, 1, c).float()).to(dt).reshape(-1)
        assert torch.equal(res[0]["y"], ref)


def _state_hash(net, opt):
    h = hashlib.sha256()  # tools/param_hash.py's hashing
    for _, v in net.state_dict().items():
        h.update(v.detach().float().cpu().numpy().tobytes())
    for a in opt.arenas():
        h.update(a.m.cpu().numpy().tobytes())
        h.update(a.v.cpu().numpy().tobytes())
    return h.hexdigest()


def _main_only_step(net, ce, opt, x, y):
    opt.zero_grad()
    (t, geo), = net.forward_lowres(x, main_only=True)
    correct = torch.empty(1, dtype=torch.int64, device=x.device)
    loss = F.upsample_cross_entropy([t], y, geo, ce.ignore_index, correct, set_correct=True)
    loss.backward()
    opt.step()
    return loss.detach(), correct


@pytest.mark.parametrize("mode", ["eager", "main_only", "graphed"])
def test_bisenet_fused_arm_bit_identical(mode):
    """BiSeNet-R18 training steps at 2x3x64x128 with fused_train on and off: losses, pixel counts
    and a hash of every parameter, buffer and Adam moment equal -- eagerly, with the main head only,
    and as hipGraph replays (which also equal the eager run)."""
    from rtsds_amd.runtime import GraphedStep
    g = torch.Generator().manual_seed(14)
    x = torch.randn(2, 3, 64, 128, generator=g).to(DEV)
    y = torch.randint(0, 20, (2, 64, 128), generator=g).to(DEV)
    ce = losses.CrossEntropyLoss(ignore_index=19)
    runs = []
    with rtsds_amd.precision(torch.bfloat16):
        for fused, graphed in ((False, False), (True, False)) + (((False, True), (True, True)) if mode == "graphed" else ()):
            AttentionRefinementModule.fused_train = fused
            try:
                torch.manual_seed(8)
                net = BiSeNet(19, "resnet18").to(DEV).train()
                opt = optim.Adam(net.parameters(), lr=1e-3)
                if mode == "main_only":
                    core = lambda: _main_only_step(net, ce, opt, x, y)  # noqa: E731
                else:
                    core = lambda: rtrain.seg_step(net, ce, opt, x, y)  # noqa: E731
                # eager: two steps; graphed: GraphedStep's own eager warm-up step, then one replay
                step = GraphedStep(core, [opt], warmup=1) if graphed else core
                ls = [[float(v) for v in step()] for _ in range(1 if graphed else 2)]
                torch.cuda.synchronize()
                runs.append((ls, _state_hash(net, opt)))
            finally:
                AttentionRefinementModule.fused_train = True
    for ls, hsh in runs[1:]:
        assert ls == runs[0][0][-len(ls):]
        assert hsh == runs[0][1]
    assert all(c > 0 for _, c in runs[0][0])
