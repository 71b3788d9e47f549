"""Fused BatchNorm-backward apply + image-conv weight gradient (rtsds_imgconv_bn_wgrad).

Op level: the fused entry against today's chain (rtsds_bn_bwd writing dx, then
rtsds_conv2d_wgrad) on the same inputs, both measured against an fp64 reference built from the
bf16 dx the chain produced (torch.nn.grad.conv2d_weight in float64 on the device).

    err = max|dW - dW64| / max|dW64|,   required: err_fused <= 2 * err_unfused

Both are fp32 sums of the same exact bf16 products in a different order -- independent draws of
the same size, hence the factor 2 and no absolute floor.  dgamma / dbeta of the coefficient-only
BatchNorm entry must equal rtsds_bn_bwd's bit for bit, two fused runs and the deferred / immediate
reductions must agree bit for bit.

Model level: one BiSeNet-R18 training step with the link on and off.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from oracle.weights import apply_recipe, synthetic_images, synthetic_labels  # noqa: E402
from rtsds_amd import _lib, losses, optim  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import train as rtrain  # noqa: E402
from rtsds_amd._lib import BF16, ConvDesc, SplitReduceDesc, lib  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402

DEV = "cuda"
K = 64
EPS = 1e-5


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)


def _desc(n, h, w, kh, pad, k=K):
    ho, wo = (h + 2 * pad - kh) // 2 + 1, (w + 2 * pad - kh) // 2 + 1
    return ConvDesc(n, h, w, 3, ho, wo, k, kh, kh, 2, 2, pad, pad, 1, 1, BF16)


def _rel_err(dw, ref):
    return ((dw.double() - ref).abs().max() / ref.abs().max()).item()


_CASES = {}


def _case(n, h, w, kh, act):
    """Inputs, today's chain and the fp64 reference of one case, computed once and left unchanged."""
    key = (n, h, w, kh, act)
    if key in _CASES:
        return _CASES[key]
    pad = kh // 2
    d = _desc(n, h, w, kh, pad)
    rows = n * d.ho * d.wo
    gen = torch.Generator(device="cpu").manual_seed(1000 * kh + 10 * h + w + act)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    img = rnd(n, h, w, 3).to(DEV, torch.bfloat16)                    # NHWC
    x = (1.5 * rnd(rows, K) + 0.5 * rnd(1, K)).to(DEV, torch.bfloat16)  # the BatchNorm's input
    g = rnd(rows, K).to(DEV, torch.bfloat16)                          # its incoming gradient
    gamma = (1.0 + 0.5 * rnd(K)).to(DEV)
    beta = (0.5 * rnd(K)).to(DEV)
    xf = x.float()
    sm = xf.mean(0).contiguous()
    si = (1.0 / torch.sqrt(xf.var(0, unbiased=False) + EPS)).contiguous()
    # today's chain
    dx = torch.empty_like(x)
    dg, db = torch.empty(K, device=DEV), torch.empty(K, device=DEV)
    ws = _ws(lib.rtsds_bn_workspace(rows, K))
    lib.rtsds_bn_bwd(_p(g), _p(x), None, _p(dx), None, _p(dg), _p(db), rows, K, _p(gamma), _p(beta), _p(sm), _p(si),
                     1, act, 0, BF16, _p(ws), ws.numel(), _stream())
    dw_unf = torch.empty(K, kh, kh, 3, device=DEV)
    ws = _ws(lib.rtsds_conv2d_wgrad_workspace(ctypes.byref(d)))
    lib.rtsds_conv2d_wgrad(ctypes.byref(d), _p(img), _p(dx), _p(dw_unf), None, 0, _p(ws), ws.numel(), _stream())
    # fp64 reference from the bf16 dx of the chain
    ref = torch.nn.grad.conv2d_weight(img.double().permute(0, 3, 1, 2), (K, 3, kh, kh),
                                      dx.double().view(n, d.ho, d.wo, K).permute(0, 3, 1, 2), stride=2, padding=pad)
    ref = ref.permute(0, 2, 3, 1).contiguous()                        # [k][kh][kw][3] like dw
    torch.cuda.synchronize()
    c = dict(d=d, rows=rows, img=img, x=x, g=g, gamma=gamma, beta=beta, sm=sm, si=si, dg=dg, db=db, dx=dx,
             dw_unf=dw_unf, ref=ref, act=act, kh=kh)
    _CASES[key] = c
    return c


def _coef(c, dg, db, accumulate=0):
    coef = torch.empty(6 * K, device=DEV)
    ws = _ws(lib.rtsds_bn_workspace(c["rows"], K))
    lib.rtsds_bn_bwd_coef(_p(c["g"]), _p(c["x"]), _p(dg), _p(db), _p(coef), c["rows"], K, _p(c["gamma"]), _p(c["beta"]),
                          _p(c["sm"]), _p(c["si"]), 1, c["act"], accumulate, BF16, _p(ws), ws.numel(), _stream())
    return coef


def _fused(c, coef, dw, accumulate=0, deferred=False):
    d = c["d"]
    ws = _ws(lib.rtsds_imgconv_bn_wgrad_workspace(ctypes.byref(d)))
    if deferred:
        pend = SplitReduceDesc()
        lib.rtsds_imgconv_bn_wgrad_deferred(ctypes.byref(d), _p(c["img"]), _p(c["g"]), _p(c["x"]), _p(coef), c["act"], _p(dw),
                                            accumulate, _p(ws), ws.numel(), ctypes.byref(pend), _stream())
        assert pend.nv > 0 and pend.dw == dw.data_ptr()
        lib.rtsds_split_reduce_many(1, (SplitReduceDesc * 1)(pend), _stream())
    else:
        lib.rtsds_imgconv_bn_wgrad(ctypes.byref(d), _p(c["img"]), _p(c["g"]), _p(c["x"]), _p(coef), c["act"], _p(dw), accumulate,
                                   _p(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    return dw


def _check(c, what):
    kh = c["kh"]
    dg, db = torch.empty(K, device=DEV), torch.empty(K, device=DEV)
    coef = _coef(c, dg, db)
    dw = _fused(c, coef, torch.full((K, kh, kh, 3), float("nan"), device=DEV))
    # 1. the BatchNorm's parameter gradients are rtsds_bn_bwd's
    assert torch.equal(dg, c["dg"]) and torch.equal(db, c["db"]), what
    # 2. run to run, 3. deferred against immediate reduce
    again = _fused(c, coef, torch.full((K, kh, kh, 3), float("nan"), device=DEV))
    assert torch.equal(dw, again), what
    later = _fused(c, coef, torch.full((K, kh, kh, 3), float("nan"), device=DEV), deferred=True)
    assert torch.equal(dw, later), what
    # 4. accuracy against the chain's
    ef, eu = _rel_err(dw, c["ref"]), _rel_err(c["dw_unf"], c["ref"])
    print(f"{what}: err_fused {ef:.3e} err_unfused {eu:.3e}")
    assert eu > 0.0, f"{what}: the unfused chain is exact here; enlarge the case"
    assert ef <= 2.0 * eu, f"{what}: err_fused {ef:.3e} > 2 x err_unfused {eu:.3e}"
    return dw, coef


SHAPES = [(1, 6, 8),        # less than one tile
          (2, 18, 136),     # output 9 x 68: partial row tile and partial column tile
          (2, 19, 136),     # odd height
          (4, 256, 1024)]   # 1,024 tiles: more than the resident workgroup slots


@pytest.mark.parametrize("kh", [7, 3])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_fused_matches_chain_relu(n, h, w, kh):
    _check(_case(n, h, w, kh, 1), f"{kh}x{kh} {n}x3x{h}x{w} relu")


@pytest.mark.parametrize("kh", [7, 3])
def test_fused_matches_chain_no_activation(kh):
    _check(_case(2, 18, 136, kh, 0), f"{kh}x{kh} 2x3x18x136 no act")


@pytest.mark.parametrize("kh", [7, 3])
def test_accumulate_onto_nonzero_dw(kh):
    c = _case(2, 19, 136, kh, 1)
    dw, coef = _check(c, f"{kh}x{kh} 2x3x19x136 relu (accumulate base)")
    base = torch.randn(K, kh, kh, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    for deferred in (False, True):
        acc = _fused(c, coef, base.clone(), accumulate=1, deferred=deferred)
        assert torch.equal(acc, base + dw), (kh, deferred)  # one fp32 add of the same reduced sum


def test_unsupported_geometry_launches_nothing():
    raw = _lib.load()
    c = _case(2, 18, 136, 3, 1)
    coef = torch.zeros(6 * K, device=DEV)
    for d in (_desc(2, 18, 136, 3, 1, k=32),   # 32 output channels
              _desc(2, 18, 135, 3, 1)):        # odd width
        assert raw.rtsds_imgconv_bn_wgrad_workspace(ctypes.byref(d)) == 0
        dw = torch.full((d.k, 3, 3, 3), 7.0, device=DEV)
        ws = _ws(1 << 20)
        ws.fill_(3)
        rc = raw.rtsds_imgconv_bn_wgrad(ctypes.byref(d), _p(c["img"]), _p(c["g"]), _p(c["x"]), _p(coef), 1, _p(dw), 0, _p(ws),
                                        ws.numel(), _stream())
        torch.cuda.synchronize()
        assert rc == 2  # RTSDS_ERR_UNSUPPORTED
        assert bool((dw == 7.0).all()) and bool((ws == 3).all())


# ----------------------------------------------------------------------------- model level
def _image_convs(net):
    return {"stem": net.context_path.conv1, "spatial": net.saptial_path.convblock1.conv1}


def _step(link_on, capture=False):
    """One seg_step of BiSeNet-R18 (train mode, bf16, 2x3x64x128): loss, correct, running statistics,
    parameter gradients, the number of fused weight-gradient calls and -- capture -- per image conv
    its (bf16 image, dx), from a tensor hook on the conv output."""
    x = synthetic_images(2, 64, 128, seed=42).to(DEV)
    y = synthetic_labels(2, 64, 128, seed=43).to(DEV)
    ce = losses.CrossEntropyLoss(ignore_index=19)
    seen, handles, calls = {}, [], []
    old, fused = F.IMG_WGRAD_LINK, F._img_bn_wgrad

    def counted(*a):
        calls.append(a[0].kh)
        return fused(*a)
    F.IMG_WGRAD_LINK, F._img_bn_wgrad = link_on, counted
    try:
        with rtsds_amd.precision(torch.bfloat16):
            net = apply_recipe(BiSeNet(19, "resnet18"), seed=1).to(DEV).train()
            opt = optim.Adam(net.parameters(), lr=1e-4)
            if capture:
                for name, conv in _image_convs(net).items():
                    def hook(mod, inp, out, name=name):
                        seen[name] = [inp[0].detach().double(), None]
                        out.register_hook(lambda gr, name=name: seen[name].__setitem__(1, gr.detach().double()))
                    handles.append(conv.register_forward_hook(hook))
            loss, correct = rtrain.seg_step(net, ce, opt, x, y)
            torch.cuda.synchronize()
    finally:
        F.IMG_WGRAD_LINK, F._img_bn_wgrad = old, fused
        for hd in handles:
            hd.remove()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    stats = {k: v.detach().clone() for k, v in net.named_buffers()}
    return dict(loss=loss.clone(), correct=correct.clone(), grads=grads, stats=stats, seen=seen, net=net, calls=calls)


def _two_steps(graphed):
    """Two seg_steps with the link on, the second eager or a GraphedStep replay; the state after."""
    from rtsds_amd.runtime import GraphedStep
    x = synthetic_images(2, 64, 128, seed=42).to(DEV)
    y = synthetic_labels(2, 64, 128, seed=43).to(DEV)
    ce = losses.CrossEntropyLoss(ignore_index=19)
    with rtsds_amd.precision(torch.bfloat16):
        net = apply_recipe(BiSeNet(19, "resnet18"), seed=1).to(DEV).train()
        opt = optim.Adam(net.parameters(), lr=1e-4)

        def core():
            return rtrain.seg_step(net, ce, opt, x, y)
        core()
        run = GraphedStep(core, [opt], warmup=0) if graphed else core
        loss, correct = run()
        torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    return loss.clone(), correct.clone(), state, grads


def test_bisenet_step_link_on_equals_off():
    assert F.IMG_WGRAD_LINK
    off = _step(False, capture=True)
    on = _step(True)
    assert off["calls"] == [] and sorted(on["calls"]) == [3, 7]  # both image convs took the fused entry
    assert torch.equal(on["loss"], off["loss"]) and torch.equal(on["correct"], off["correct"])
    for k in off["stats"]:
        assert torch.equal(on["stats"][k], off["stats"][k]), k
    fused_names = {k for k, p in off["net"].named_parameters()
                   if any(p is conv.weight for conv in _image_convs(off["net"]).values())}
    assert len(fused_names) == 2, fused_names
    assert set(on["grads"]) == set(off["grads"])
    for k in off["grads"]:
        if k not in fused_names:
            assert torch.equal(on["grads"][k], off["grads"][k]), k
    # the two image convs: both paths against fp64 from the dx the separate apply pass wrote
    for name, conv in _image_convs(off["net"]).items():
        pname = next(k for k, p in off["net"].named_parameters() if p is conv.weight)
        img, dx = off["seen"][name]
        assert dx is not None, name
        kh = conv.kernel_size[0]
        ref = torch.nn.grad.conv2d_weight(img, (K, 3, kh, kh), dx, stride=2, padding=conv.padding[0])
        ef, eu = _rel_err(on["grads"][pname], ref), _rel_err(off["grads"][pname], ref)
        print(f"model {name}: err_fused {ef:.3e} err_unfused {eu:.3e}")
        assert not torch.equal(on["grads"][pname], torch.zeros_like(on["grads"][pname]))
        assert eu > 0.0, name
        assert ef <= 2.0 * eu, f"{name}: err_fused {ef:.3e} > 2 x err_unfused {eu:.3e}"


def test_bisenet_step_link_graph_replay_equals_eager():
    assert F.IMG_WGRAD_LINK
    el, ec, es, eg = _two_steps(False)
    gl, gc, gs, gg = _two_steps(True)
    assert torch.equal(el, gl) and torch.equal(ec, gc)
    for k in es:
        assert torch.equal(es[k], gs[k]), k
    for k in eg:
        assert torch.equal(eg[k], gg[k]), k
