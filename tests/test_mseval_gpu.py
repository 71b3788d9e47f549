"""Multi-scale / flip evaluation (rtsds_upsoftmax_acc, functional.upsample_softmax_accumulate,
validation.predict_multiscale, val(scales=, flip=)).  GPU only.

Op level: the fp32 probabilities are pinned bit for bit to functional.upsample_softmax (and to
torch fp64 with that op's tolerance), the mirrored store to torch.flip, the accumulation to a
plain fp32 add (an FMA of z * (1/sum) + acc would differ), the argmax to first-max-wins, and a
captured replay to the eager result.  End to end: BiSeNet-R18 in fp32 mode against the CPU
oracle evaluated scale by scale, and DeepLabV2 against the same sequence of unfused ops.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from oracle import models as om  # noqa: E402
from oracle.weights import recipe_state_dict, synthetic_images, synthetic_labels  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import utils, validation  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402
from rtsds_amd.models.deeplabv2.deeplabv2 import get_deeplab_v2  # noqa: E402

DEV = "cuda"
CL = torch.channels_last
NC = 19
TOL = {torch.float32: 2e-4, torch.bfloat16: 3e-2}  # test_upsample_softmax_fused's tolerance for y
GEOS = [
    ((2, 19, 16, 32), (128, 256)),   # the three of test_upsample_softmax_fused
    ((1, 19, 13, 17), (97, 129)),
    ((2, 7, 9, 40), (64, 96)),
    ((1, 19, 8, 40), (24, 300)),     # two column tiles, ragged last tile, x7.5: mirrored tile write
    ((2, 19, 6, 12), (64, 128)),     # x10.67 (scale 0.75)
    ((2, 19, 12, 24), (64, 128)),    # x5.33 (scale 1.5)
]
DTS = [torch.float32, torch.bfloat16]
geos = pytest.mark.parametrize("geo", GEOS, ids=lambda g: "x".join(map(str, g[0])) + "-" + "x".join(map(str, g[1])))
dts = pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])


def _logits(geo, dt, extra=0):
    (n, c, h, w), _ = geo
    g = torch.Generator().manual_seed(n * 7 + h + 1000 * extra)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 3
    return x.bfloat16().double() if dt == torch.bfloat16 else x


def _dev(t, dt):
    return t.to(DEV, dt).contiguous(memory_format=CL)


def _nan_acc(geo):
    (n, c, _, _), (ho, wo) = geo
    return torch.full((n, ho, wo, c), float("nan"), dtype=torch.float32, device=DEV)


def _probs(xd, geo, flip=False):
    """One overwrite pass into a NaN-filled acc (an unwritten element would stay NaN)."""
    acc = _nan_acc(geo)
    out = F.upsample_softmax_accumulate(xd, F.upsample_geometry(xd, size=geo[1]), acc, flip=flip, accumulate=False)
    assert out is acc
    return acc


def _first_max(acc):
    """First-max index over the last dim, on the host."""
    a = acc.cpu()
    c = a.shape[-1]
    return torch.where(a == a.max(-1, keepdim=True).values, torch.arange(c), torch.tensor(c)).min(-1).values


@dts
@geos
def test_overwrite_matches_upsample_softmax(geo, dt):
    x = _logits(geo, dt)
    xd = _dev(x, dt)
    acc = _probs(xd, geo)
    y = F.upsample_softmax(xd, F.upsample_geometry(xd, size=geo[1]))
    got = acc.permute(0, 3, 1, 2)
    assert torch.equal(got if dt == torch.float32 else got.to(torch.bfloat16), y)
    ref = torch.softmax(TF.interpolate(x, size=geo[1], mode="bilinear", align_corners=False), dim=1)
    err = (got.double().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-12
    assert err <= TOL[dt] * scale + 1e-6, (err, scale)


@dts
@geos
def test_flip_stores_mirrored(geo, dt):
    xd = _dev(_logits(geo, dt), dt)
    assert torch.equal(_probs(xd, geo, flip=True), torch.flip(_probs(xd, geo, flip=False), dims=[2]))


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@dts
@geos
def test_accumulate_is_one_fp32_add(geo, dt, flip):
    """acc + p with p the already rounded product z * (1/sum): a contracted FMA differs."""
    xd = _dev(_logits(geo, dt), dt)
    p = _probs(xd, geo, flip=flip)
    g = torch.Generator().manual_seed(11)
    acc0 = (torch.rand(p.shape, generator=g, dtype=torch.float32) * 5).to(DEV)
    acc = acc0.clone()
    F.upsample_softmax_accumulate(xd, F.upsample_geometry(xd, size=geo[1]), acc, flip=flip, accumulate=True)
    assert torch.equal(acc, acc0 + p)


@dts
@geos
def test_four_passes_match_unfused_chain(geo, dt):
    """Plain and flipped passes of two inputs vs upsample_softmax -> fp32 -> flip -> + on the
    device.  fp32: identical.  bf16: the chain rounds each probability <= 1 to bf16, a half-ulp
    of at most 2^-9 per pass."""
    xs = [_dev(_logits(geo, dt, e), dt) for e in (0, 1)]
    passes = [(xs[0], False), (xs[0], True), (xs[1], False), (xs[1], True)]
    acc = _nan_acc(geo)
    chain = None
    for i, (xd, flip) in enumerate(passes):
        gm = F.upsample_geometry(xd, size=geo[1])
        F.upsample_softmax_accumulate(xd, gm, acc, flip=flip, accumulate=i > 0)
        p = F.upsample_softmax(xd, gm).float()
        if flip:
            p = torch.flip(p, dims=[3])
        p = p.permute(0, 2, 3, 1)
        chain = p.clone() if chain is None else chain + p
    if dt == torch.float32:
        assert torch.equal(acc, chain)
    else:
        err = (acc - chain).abs().max().item()
        print(f"bf16 4-pass |fused - chain| max {err:.3e} (bound {4 * 2.0 ** -9:.3e})")
        assert err <= 4 * 2.0 ** -9, err


@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@dts
@geos
def test_pred_is_first_max_of_acc(geo, dt, ties):
    (n, c, h, w), (ho, wo) = geo
    x = _logits(geo, dt)
    if ties:  # two classes with identical logits everywhere, above all others: the lower index wins
        top = x.max(dim=1).values + 0.5
        x[:, 2] = top
        x[:, 5] = top
        if dt == torch.bfloat16:
            x = x.bfloat16().double()
    xd = _dev(x, dt)
    gm = F.upsample_geometry(xd, size=(ho, wo))
    acc = _nan_acc(geo)
    pred = torch.full((n, ho, wo), -1, dtype=torch.int64, device=DEV)
    F.upsample_softmax_accumulate(xd, gm, acc, flip=False, accumulate=False, pred=pred)
    assert torch.equal(pred.cpu(), _first_max(acc))
    if ties:
        assert int(pred.min()) == 2 and int(pred.max()) == 2
    # second, mirrored pass of another input: pred follows the updated sum at the mirrored column
    x2 = _dev(_logits(geo, dt, 1), dt)
    pred.fill_(-1)
    F.upsample_softmax_accumulate(x2, gm, acc, flip=True, accumulate=True, pred=pred)
    assert torch.equal(pred.cpu(), _first_max(acc))


@dts
def test_graph_capture_replay_equals_eager(dt):
    geo = GEOS[3]
    (n, c, _, _), (ho, wo) = geo
    xa, xb = _dev(_logits(geo, dt), dt), _dev(_logits(geo, dt, 1), dt)
    gm = F.upsample_geometry(xa, size=(ho, wo))

    def two_passes(acc, pred):
        F.upsample_softmax_accumulate(xa, gm, acc, flip=False, accumulate=False)
        F.upsample_softmax_accumulate(xb, gm, acc, flip=True, accumulate=True, pred=pred)

    acc_e, pred_e = _nan_acc(geo), torch.full((n, ho, wo), -1, dtype=torch.int64, device=DEV)
    two_passes(acc_e, pred_e)
    acc_g, pred_g = _nan_acc(geo), torch.full((n, ho, wo), -1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        two_passes(acc_g, pred_g)
    acc_g.fill_(float("nan"))
    pred_g.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc_g, acc_e) and torch.equal(pred_g, pred_e)


def test_wrapper_rejects_bad_buffers():
    geo = GEOS[0]
    (n, c, _, _), (ho, wo) = geo
    xd = _dev(_logits(geo, torch.float32), torch.float32)
    gm = F.upsample_geometry(xd, size=(ho, wo))
    good = torch.zeros((n, ho, wo, c), dtype=torch.float32, device=DEV)
    bad = [good.to(torch.bfloat16), torch.zeros((n, c, ho, wo), dtype=torch.float32, device=DEV),
           torch.zeros((n, ho, wo, 32), dtype=torch.float32, device=DEV)[..., :c], torch.zeros((n, ho, wo, c))]
    for acc in bad:
        with pytest.raises(RuntimeError, match="acc must be"):
            F.upsample_softmax_accumulate(xd, gm, acc)
    for pred in (torch.zeros((n, ho, wo), dtype=torch.int32, device=DEV),
                 torch.zeros((n, wo, ho), dtype=torch.int64, device=DEV)):
        with pytest.raises(RuntimeError, match="pred must be"):
            F.upsample_softmax_accumulate(xd, gm, good, pred=pred)
    torch.cuda.synchronize()
    assert float(good.abs().max()) == 0.0  # nothing was launched on the valid buffer


# ----------------------------------------------------------------------------- end to end
SCALES, SIZE = (0.5, 1.0, 1.5), (128, 256)


def _load(model, seed):
    sd = model.state_dict()
    model.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed))
    return model


@pytest.fixture(scope="module")
def bisenet_ms():
    """Oracle BiSeNet-R18 (recipe seed 1, BatchNorm running statistics warmed by one train-mode
    forward with momentum 1, as test_configs_gpu.eval_state), its multi-scale / flip reference
    on the CPU, and the package's model on the same state in fp32 mode.

    Reference, per scale and per flip: torch interpolate of the images, the oracle's
    low-resolution head (fusion module output -> final 1x1 conv, i.e. its forward without the
    x8 resize), interpolate to the label size, fp64 softmax, un-flip, sum."""
    ref = _load(om.BiSeNet(NC, "resnet18"), 1).train()
    bns = [m for m in ref.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = 1.0
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        ref(synthetic_images(2, *SIZE, seed=50))
    for m in bns:
        m.momentum = 0.1
    ref.eval()
    x = synthetic_images(2, *SIZE, seed=42)
    box = []
    hook = ref.feature_fusion_module.register_forward_hook(lambda mod, args, out: box.append(out))
    want = torch.zeros(2, NC, *SIZE, dtype=torch.float64)
    max_logit = 0.0
    with torch.no_grad():
        for s in SCALES:
            hw = validation.scaled_size(SIZE, s)
            xs = x if hw == SIZE else TF.interpolate(x, size=hw, mode="bilinear", align_corners=False)
            for flip in (False, True):
                box.clear()
                ref(torch.flip(xs, dims=[3]) if flip else xs)
                low = ref.conv(box[0]).double()
                max_logit = max(max_logit, low.abs().max().item())
                p = torch.softmax(TF.interpolate(low, size=SIZE, mode="bilinear", align_corners=False), dim=1)
                want += torch.flip(p, dims=[3]) if flip else p
    hook.remove()
    net = BiSeNet(NC, "resnet18")
    net.load_state_dict(ref.state_dict())
    net = net.to(DEV).eval()
    with rtsds_amd.precision(torch.float32):
        acc, pred = validation.predict_multiscale(net, x.to(DEV), SIZE, scales=SCALES, flip=True)
    torch.cuda.synchronize()
    return dict(net=net, x=x, want=want, max_logit=max_logit, acc=acc, pred=pred)


def test_bisenet_multiscale_flip_matches_oracle(bisenet_ms):
    """|acc - ref| <= 0.5 * passes * eps with eps = 1e-3 * max|reference low-res logit| (the
    project's eval-logit bound; 0.5 from the softmax Jacobian, |dp_k| <= 2 eps p_k (1 - p_k) <=
    eps / 2), and pred = the reference argmax wherever the reference top-2 gap exceeds 2 tol
    (at least 90 % of the pixels)."""
    s = bisenet_ms
    passes = 2 * len(SCALES)
    tol = 0.5 * passes * 1e-3 * s["max_logit"]
    got = s["acc"].permute(0, 3, 1, 2).double().cpu()
    assert got.shape == s["want"].shape and s["acc"].dtype == torch.float32
    err = (got - s["want"]).abs().max().item()
    top2 = s["want"].topk(2, dim=1).values
    safe = (top2[:, 0] - top2[:, 1]) > 2 * tol
    frac = float(safe.float().mean())
    mism = int(((s["pred"].cpu() != s["want"].argmax(1)) & safe).sum())
    print(f"multi-scale acc vs oracle: max|logit| {s['max_logit']:.3f}, tol {tol:.4f}, max err {err:.3e}, "
          f"safe pixels {frac:.4f}, argmax mismatches at safe pixels {mism}")
    assert err <= tol, (err, tol)
    assert frac >= 0.90, frac
    assert mism == 0, mism
    assert torch.equal(s["pred"].cpu(), _first_max(s["acc"]))


def _val_hist(monkeypatch, *args, **kw):
    """validation.val's confusion histogram (captured where val hands it to per_class_iou)."""
    seen = []
    real = utils.per_class_iou
    monkeypatch.setattr(validation.utils, "per_class_iou", lambda h: (seen.append(np.array(h)), real(h))[1])
    miou = validation.val(*args, **kw)
    return miou, seen[0]


def test_val_multiscale_histogram(bisenet_ms, monkeypatch):
    s = bisenet_ms
    y = synthetic_labels(2, *SIZE, seed=43)
    with rtsds_amd.precision(torch.float32):
        miou, hist = _val_hist(monkeypatch, 0, s["net"], [(s["x"], y)], NC, device=DEV, scales=SCALES, flip=True)
    want = torch.zeros(NC * NC, dtype=torch.int64, device=DEV)
    F.confusion(y.to(DEV), s["pred"], want, NC)
    assert np.array_equal(hist, want.view(NC, NC).cpu().numpy())
    assert hist.sum() > 0 and miou == np.nanmean(utils.per_class_iou(hist))


def test_val_default_path_untouched(bisenet_ms, monkeypatch):
    """Without the new arguments val is the single full-resolution pass (argmax of model(x)) and
    never enters predict_multiscale."""
    s = bisenet_ms
    y = synthetic_labels(2, *SIZE, seed=43)

    def boom(*a, **k):
        raise AssertionError("predict_multiscale called on the default path")
    monkeypatch.setattr(validation, "predict_multiscale", boom)
    with rtsds_amd.precision(torch.float32):
        miou, hist = _val_hist(monkeypatch, 0, s["net"], [(s["x"], y)], NC, device=DEV)
        with torch.no_grad():
            pred = F.argmax_channels(s["net"](s["x"].to(DEV)))
    want = torch.zeros(NC * NC, dtype=torch.int64, device=DEV)
    F.confusion(y.to(DEV), pred, want, NC)
    assert np.array_equal(hist, want.view(NC, NC).cpu().numpy())
    assert miou == np.nanmean(utils.per_class_iou(want.view(NC, NC).cpu().numpy()))


def test_deeplab_multiscale_equals_unfused_sequence():
    """predict_multiscale on DeepLabV2 (64 x 128, batch 1, fp32 mode, scales 0.5 and 1.0 with
    flip) vs the same passes built from forward_lowres and the unfused ops."""
    size, scales = (64, 128), (0.5, 1.0)
    net = _load(get_deeplab_v2(NC, pretrain=False), 3).to(DEV).eval()
    x = synthetic_images(1, *size, seed=44).to(DEV)
    with rtsds_amd.precision(torch.float32):
        acc, pred = validation.predict_multiscale(net, x, size, scales=scales, flip=True)
        chain = None
        with torch.no_grad():
            for sc in scales:
                hw = validation.scaled_size(size, sc)
                xs = x if hw == size else F.interpolate_bilinear(x, size=hw)
                for flip in (False, True):
                    (low, _), = net.forward_lowres(torch.flip(xs, dims=[3]) if flip else xs, main_only=True)
                    p = F.upsample_softmax(low, F.upsample_geometry(low, size=size)).float()
                    p = (torch.flip(p, dims=[3]) if flip else p).permute(0, 2, 3, 1)
                    chain = p.clone() if chain is None else chain + p
    assert acc.shape == (1, *size, NC) and bool(torch.isfinite(acc).all())
    assert torch.equal(acc, chain)
    assert torch.equal(pred.cpu(), _first_max(acc))


def test_predict_multiscale_single_scale_is_softmax_of_model(bisenet_ms):
    """The protocol at scales=(1.0,), flip=False is softmax(model(x)): the model resizes its head
    with the same one-step bilinear, so the logits are the same bits and only the two fp32
    softmax evaluations differ (a few ulp of values <= 1: bound 1e-5)."""
    net, x = bisenet_ms["net"], bisenet_ms["x"].to(DEV)
    with rtsds_amd.precision(torch.float32), torch.no_grad():
        acc, pred = validation.predict_multiscale(net, x, SIZE)
        logits = net(x).float()
    want = torch.softmax(logits, dim=1)
    assert (acc.permute(0, 3, 1, 2) - want).abs().max().item() <= 1e-5
    assert torch.equal(pred.cpu(), _first_max(acc))
