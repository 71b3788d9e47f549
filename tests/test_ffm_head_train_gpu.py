"""Training-mode FeatureFusionModule tail as functional.FfmTailFn (FeatureFusionModule.fused_head)
against the op-by-op chain it replaces -- BatchNormFn, GapFn, PooledMlpFn, ChScaleFn -- bit for
bit: op level on the shapes at which the kernels take another path, the fallback shapes, and one
BiSeNet-R18 training step eagerly, with the main head only, and as hipGraph replays."""
import hashlib

import pytest
import torch

import rtsds_amd
from rtsds_amd import functional as F
from rtsds_amd import losses, optim
from rtsds_amd import train as rtrain
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet, FeatureFusionModule
from rtsds_amd.nn import Conv2d

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
CIN = 16  # channels of the module's concatenated input in the op-level cases


class _Tail(torch.nn.Module):
    """The fusion module and the model's final 1x1 conv, as BiSeNet._heads chains them."""

    def __init__(self, c):
        super().__init__()
        self.ffm = FeatureFusionModule(c, CIN)
        self.conv = Conv2d(c, c, kernel_size=1)

    def forward(self, x):
        return self.conv(self.ffm(x, reader=self.conv))


def _tail_run(fused, dt, n, c, h, w, arena):
    """One forward / backward of _Tail with non-trivial parameters; every output and gradient.
    ``arena``: the parameters belong to an rtsds optimizer, so the weight gradients accumulate
    into its (pre-filled) gradient buffers."""
    FeatureFusionModule.fused_head = fused
    try:
        with rtsds_amd.precision(dt):
            torch.manual_seed(31)
            m = _Tail(c).to(DEV).train()
            g = torch.Generator().manual_seed(32)
            with torch.no_grad():
                for p in m.parameters():
                    if p.dim() == 1:  # biases, BatchNorm weight / bias
                        p.copy_(torch.randn(p.shape, generator=g).to(DEV) * 0.5 + (1.0 if p is m.ffm.convblock.bn.weight else 0.0))
            opt = None
            if arena:
                opt = optim.Adam(m.parameters(), lr=1e-3)
                for a in opt.arenas():
                    a.gflat.copy_(torch.randn(a.gflat.shape, generator=g).to(DEV))
            x = torch.randn(n, CIN, h, w, generator=g).to(DEV, dt).contiguous(memory_format=torch.channels_last)
            x.requires_grad_()
            gy = torch.randn(n, c, h, w, generator=g).to(DEV, dt).contiguous(memory_format=torch.channels_last)
            taken = []
            orig = F.ffm_tail
            F.ffm_tail = lambda *a: (taken.append(1), orig(*a))[1]  # (did the module take the fused path?)
            try:
                y = m(x)
            finally:
                F.ffm_tail = orig
            y.backward(gy)
            torch.cuda.synchronize()
            out = {"y": y.detach(), "dx": x.grad}
            for k, p in m.named_parameters():
                out["grad." + k] = p.grad.detach().clone()
            for k, b in m.named_buffers():
                out["buf." + k] = b.detach().clone()
            return out, bool(taken)
    finally:
        FeatureFusionModule.fused_head = True


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


# 8x8: one slice, one weight-gradient block, one pixel chunk, the BatchNorm's few-row forms;
# 8x24: several slices per image, ragged last tile; 20x24: hw = 480, slices of unequal length, N
# not a power of two, two pixel chunks (the last partial); 8x32x64: N at the limit, 64 slices.
@pytest.mark.parametrize("arena", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("geo", [(1, 8, 8), (2, 8, 24), (3, 20, 24), (8, 32, 64)])
def test_ffm_tail_equals_chain(geo, dt, arena):
    """Logits, input gradient (through the BatchNorm's dx and the 3x3 conv), dgamma / dbeta, running
    statistics and the gradients of the three 1x1 convs, fused against the chain."""
    n, h, w = geo
    ref, t0 = _tail_run(False, dt, n, 19, h, w, arena)
    got, t1 = _tail_run(True, dt, n, 19, h, w, arena)
    assert not t0 and t1
    _same(ref, got)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("geo", [(1, 8, 8), (3, 20, 24), (8, 32, 64)])
def test_ffm_tail_intermediates_equal_chain(geo, dt):
    """The Function itself against the four Functions it replaces on one conv output: r, the saved
    feature / pooled / hid / att, and dx of the BatchNorm, dgamma, dbeta, dW1, db1, dW2, db2."""
    n, h, w = geo
    c = 19
    g = torch.Generator().manual_seed(5)
    x0 = (torch.randn(n, c, h, w, generator=g) * 2 + 0.3).to(DEV, dt).contiguous(memory_format=torch.channels_last)
    gam, bet = (torch.randn(c, generator=g) * 0.5 + 1).to(DEV), torch.randn(c, generator=g).to(DEV)
    ws = [(torch.randn(c, c, 1, 1, generator=g) / c ** 0.5).to(DEV).contiguous(memory_format=torch.channels_last) for _ in range(2)]
    bs = [torch.randn(c, generator=g).to(DEV) for _ in range(2)]
    dr = torch.randn(n, c, h, w, generator=g).to(DEV, dt).contiguous(memory_format=torch.channels_last)
    res = []
    for fused in (False, True):
        x = x0.clone().requires_grad_()
        ps = [t.clone().requires_grad_() for t in (gam, bet, ws[0], bs[0], ws[1], bs[1])]
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        wq = [p.detach().to(dt).contiguous(memory_format=torch.channels_last) for p in (ps[2], ps[4])]
        if fused:
            r = F.ffm_tail(x, ps[0], ps[1], rm, rv, 0.1, 1e-5, nbt, ps[2], ps[3], wq[0], ps[4], ps[5], wq[1])
            feature, pooled, hid, att = r.grad_fn.saved_tensors[1:5]
        else:
            feature = F.batch_norm(x, ps[0], ps[1], rm, rv, True, 0.1, 1e-5, act=1, num_batches_tracked=nbt)
            join = F.GradJoin(2)
            pooled = F.global_avg_pool(feature, join)
            att = F.pooled_mlp(pooled, ps[2], ps[3], wq[0], ps[4], ps[5], wq[1])
            hid = att.grad_fn.saved_tensors[1]
            r = F.channel_scale(feature, att, residual=True, join=join)
        r.backward(dr)
        torch.cuda.synchronize()
        out = {"r": r.detach(), "feature": feature.detach(), "pooled": pooled.detach(), "hid": hid.detach(),
               "att": att.detach(), "dx": x.grad, "rm": rm, "rv": rv, "nbt": nbt}
        out.update({f"g{i}": p.grad for i, p in enumerate(ps)})
        res.append(out)
    _same(res[0], res[1])


@pytest.mark.parametrize("geo", [(2, 21, 8, 8), (2, 19, 5, 7), (9, 19, 8, 8)])
def test_ffm_tail_fallback(geo):
    """Another class count, hw off the vector width, N past the pooled kernels' limit: the chain
    runs, with the chain's results, and nothing raises."""
    n, c, h, w = geo
    ref, t0 = _tail_run(False, torch.bfloat16, n, c, h, w, False)
    got, t1 = _tail_run(True, torch.bfloat16, n, c, h, w, False)
    assert not t0 and not t1
    _same(ref, got)


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
    heads = net.forward_lowres(x, main_only=True)
    (t, geo), = heads
    correct = torch.empty(1, dtype=torch.int64, device=x.device)
    loss = F.upsample_cross_entropy([t], y, geo, ce.ignore_index, correct, set_correct=True)
    loss.backward()
    opt.step()
    return loss.detach(), correct


@pytest.mark.parametrize("mode", ["eager", "main_only", "graphed"])
def test_bisenet_fused_head_bit_identical(mode):
    """BiSeNet-R18 training steps at 2x3x64x128 with fused_head on and off: losses, pixel counts
    and a hash of every parameter, buffer and Adam moment equal -- eagerly, with the main head only
    (the DA target branch's call), and as hipGraph replays (which also equal the eager run)."""
    from rtsds_amd.runtime import GraphedStep
    g = torch.Generator().manual_seed(14)
    x = torch.randn(2, 3, 64, 128, generator=g).to(DEV)
    y = torch.randint(0, 20, (2, 64, 128), generator=g).to(DEV)
    ce = losses.CrossEntropyLoss(ignore_index=19)
    runs = []
    with rtsds_amd.precision(torch.bfloat16):
        for fused, graphed in ((False, False), (True, False)) + (((False, True), (True, True)) if mode == "graphed" else ()):
            FeatureFusionModule.fused_head = fused
            try:
                torch.manual_seed(8)
                net = BiSeNet(19, "resnet18").to(DEV).train()
                opt = optim.Adam(net.parameters(), lr=1e-3)
                if mode == "main_only":
                    core = lambda: _main_only_step(net, ce, opt, x, y)  # noqa: E731
                else:
                    core = lambda: rtrain.seg_step(net, ce, opt, x, y)  # noqa: E731
                # three steps; graphed: GraphedStep's own eager warm-up step (not returned), then two replays
                step = GraphedStep(core, [opt], warmup=1) if graphed else core
                ls = [[float(v) for v in step()] for _ in range(2 if graphed else 3)]
                torch.cuda.synchronize()
                runs.append((ls, _state_hash(net, opt)))
            finally:
                FeatureFusionModule.fused_head = True
    for ls, hsh in runs[1:]:
        assert ls == runs[0][0][-len(ls):]
        assert hsh == runs[0][1]
    assert all(c > 0 for _, c in runs[0][0])
