"""Class-balanced pseudo-labels on the device (rtsds_conf_hist, rtsds_pseudo_select,
functional.confidence_histogram / pseudo_select, rtsds_amd.selftrain, main --self_training).

Every comparison in this file is EXACT: the reference is computed on the host from ``acc.cpu()``
with the same fp32 operations (first maximum, one multiply by float32(1 / passes), one multiply
by bins -- a power of two, so exact -- floor, clamp) and integer counts."""
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from oracle.weights import recipe_state_dict, synthetic_images  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import losses, optim, selftrain, train, validation  # noqa: E402
from rtsds_amd import main as rmain  # noqa: E402
from rtsds_amd.callbacks import Callback  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402

DEV = torch.device("cuda", 0)
IGNORE = 19


# ----------------------------------------------------------------------------- host reference
def host_ref(acc, bins, passes):
    """(hist [c, bins], pred [n, H, W], cbin [n, H, W]) as int64 numpy, from acc.cpu()."""
    a = acc.detach().cpu().numpy()
    assert a.dtype == np.float32
    shape, c = a.shape[:-1], a.shape[-1]
    a = a.reshape(-1, c)
    nan = np.isnan(a)
    # first maximum; a NaN beats every number and the first NaN wins (rtsds_argmax's rule)
    k = np.where(nan.any(1), nan.argmax(1), np.where(nan, -np.inf, a).argmax(1))
    best = a[np.arange(a.shape[0]), k]
    inv = np.float32(1.0) / np.float32(passes)
    with np.errstate(invalid="ignore", over="ignore"):
        conf = (best * inv).astype(np.float32)
        t = np.floor((conf * np.float32(bins)).astype(np.float32))
        b = np.where(conf > 0, np.minimum(t, bins - 1), 0)
    b = np.nan_to_num(b, nan=0.0).astype(np.int64)
    hist = np.bincount(k * bins + b, minlength=c * bins).reshape(c, bins)
    return hist, k.reshape(shape), b.reshape(shape)


def _u16(shape, value):
    return torch.from_numpy(np.full(shape, value, dtype=np.uint16)).to(DEV)


def _np(t):
    return t.cpu().numpy().astype(np.int64)


def run_hist(acc, bins, passes, hist=None, want_pred=True, want_cbin=True):
    n, h, w, c = acc.shape
    if hist is None:
        hist = torch.zeros((c, bins), dtype=torch.int64, device=DEV)
    pred = torch.full((n, h, w), 0xFF, dtype=torch.uint8, device=DEV) if want_pred else None
    cbin = _u16((n, h, w), 0xFFFF) if want_cbin else None
    out = F.confidence_histogram(acc, hist, passes=passes, pred=pred, cbin=cbin)
    assert out is hist
    return hist, pred, cbin


def check(acc, bins, passes):
    hist, pred, cbin = run_hist(acc, bins, passes)
    rh, rp, rb = host_ref(acc, bins, passes)
    assert np.array_equal(_np(pred), rp)       # no 0xFF sentinel can survive: classes are < 32
    assert np.array_equal(_np(cbin), rb)       # nor 0xFFFF: bins are < 1024
    assert np.array_equal(_np(hist), rh)
    assert int(hist.sum()) == rp.size
    return hist, pred, cbin, (rh, rp, rb)


# ----------------------------------------------------------------------------- inputs
def softmax_sum(shape, passes, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    acc = torch.zeros(shape, dtype=torch.float32, device=DEV)
    for _ in range(passes):
        acc += torch.softmax(3 * torch.randn(shape, generator=g, device=DEV), dim=-1)
    return acc.contiguous()


def one_hot(shape, passes, seed=1, single=None):
    """Exactly ``passes`` at one class per pixel: conf reaches (passes 1, 2) or rounds to
    (passes 6: 6 * float32(1/6)) 1.0, which must clamp into the top bin; every lane of a wave hits
    the same few cells (``single``: one cell), the worst case for the LDS atomics."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    k = torch.full(shape[:-1], single, device=DEV) if single is not None else \
        torch.randint(0, shape[-1], shape[:-1], generator=g, device=DEV)
    return (torch.nn.functional.one_hot(k, shape[-1]).float() * passes).contiguous()


SMALL = [(1, 13, 17, 19),    # fewer pixels than one block, unaligned rows
         (2, 24, 300, 19),   # many blocks, ragged tail
         (2, 9, 40, 7),      # few classes
         (1, 16, 32, 32),    # the class cap
         (1, 8, 8, 2)]       # the class floor
BIG = (2, 512, 1024, 19)     # more pixels than one pass of the launch grid
# (bins, passes); 32 classes x 1024 bins does not fit the LDS budget (test_pseudo_cpu)
COMBOS = [(16, 1), (256, 2), (1024, 6), (1024, 1), (16, 6)]


def _combos(shape):
    return [(b, p) for b, p in COMBOS if not (shape[-1] > 26 and b == 1024)]


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_conf_hist_softmax_equals_host(shape):
    for bins, passes in _combos(shape):
        check(softmax_sum(shape, passes, seed=bins + passes), bins, passes)


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_conf_hist_one_hot_clamps_to_top_bin(shape):
    for bins, passes in _combos(shape):
        hist, pred, cbin, _ = check(one_hot(shape, passes), bins, passes)
        assert int(_np(cbin).min()) == bins - 1 and int(hist[:, :-1].sum()) == 0
        hist, *_ = check(one_hot(shape, passes, single=shape[-1] - 1), bins, passes)
        assert int(hist[-1, -1]) == shape[0] * shape[1] * shape[2]


@pytest.mark.parametrize("bins,passes", [(1024, 6), (256, 1)])
def test_conf_hist_big_softmax_and_single_cell(bins, passes):
    """Grid-stride loop (more tiles than workgroups) and the 64-bit flush; the one-class input
    puts 2^20 pixels into a single cell."""
    check(softmax_sum(BIG, passes, seed=7), bins, passes)
    hist, *_ = check(one_hot(BIG, passes, single=3), bins, passes)
    assert int(hist[3, bins - 1]) == BIG[0] * BIG[1] * BIG[2]


def test_conf_hist_ties_zeros_nan():
    shape = (2, 9, 40, 7)
    acc = softmax_sum(shape, 1, seed=5)
    acc[..., 5] = acc[..., 2] = 0.5 + acc.max(dim=-1).values  # two equal maxima: the first (2) wins
    _, pred, _, _ = check(acc, 256, 1)
    assert int(pred.min()) == 2 and int(pred.max()) == 2
    hist, pred, cbin, _ = check(torch.zeros(shape, device=DEV), 256, 2)  # all zeros: class 0, bin 0
    assert int(pred.max()) == 0 and int(_np(cbin).max()) == 0 and int(hist[0, 0]) == 2 * 9 * 40
    acc = softmax_sum(shape, 1, seed=6)
    acc[0, :, ::3, 4] = float("nan")  # a NaN is the maximum; its confidence is not > 0: bin 0
    acc[0, :, ::6, 6] = float("nan")  # the first NaN wins
    acc[1, 0, :, 0] = -1.0
    acc[1, 0, :, 1:] = -2.0           # a negative maximum: bin 0
    _, pred, cbin, _ = check(acc, 16, 1)
    assert int(pred[0, 0, 0]) == 4 and int(_np(cbin)[0, 0, 0]) == 0
    assert int(pred[1, 0, 0]) == 0 and int(_np(cbin)[1, 0, 0]) == 0


@pytest.mark.parametrize("shape,bins", [((1, 13, 17, 19), 1024), ((2, 24, 300, 19), 16), ((2, 9, 40, 7), 256)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conf_hist_unaligned_acc(shape, bins):
    """acc 4 bytes off a 16-B boundary (a contiguous view into a larger buffer): the kernel's
    plain staged loop instead of the register-prefetched one; same results."""
    src = softmax_sum(shape, 2, seed=9)
    flat = torch.empty(src.numel() + 1, dtype=torch.float32, device=DEV)
    acc = flat[1:].view(shape)
    acc.copy_(src)
    assert acc.is_contiguous() and acc.data_ptr() % 16 == 4
    check(acc, bins, 2)
    check(acc.copy_(one_hot(shape, 2)), bins, 2)


def test_conf_hist_accumulates_and_optional_outputs():
    shape, bins = (2, 24, 300, 19), 256
    a, b = softmax_sum(shape, 2, seed=11), softmax_sum(shape, 2, seed=12)
    ra, rb = host_ref(a, bins, 2)[0], host_ref(b, bins, 2)[0]
    pre = torch.arange(19 * bins, dtype=torch.int64, device=DEV).view(19, bins) * 3 + 1
    hist = pre.clone()
    run_hist(a, bins, 2, hist=hist)
    assert np.array_equal(_np(hist), _np(pre) + ra)      # added to, not cleared
    run_hist(b, bins, 2, hist=hist, want_pred=False)     # two calls give the sum; pred=None
    assert np.array_equal(_np(hist), _np(pre) + ra + rb)
    _, pred, cbin = run_hist(a, bins, 2, hist=hist, want_cbin=False)
    assert cbin is None and np.array_equal(_np(pred), host_ref(a, bins, 2)[1])
    _, pred, cbin = run_hist(a, bins, 2, hist=hist, want_pred=False)
    assert pred is None and np.array_equal(_np(cbin), host_ref(a, bins, 2)[2])
    run_hist(a, bins, 2, hist=hist, want_pred=False, want_cbin=False)
    assert np.array_equal(_np(hist), _np(pre) + 4 * ra + rb)
    big = torch.full((19, bins), 1 << 40, dtype=torch.int64, device=DEV)  # 64-bit cells
    run_hist(a, bins, 2, hist=big)
    assert np.array_equal(_np(big), (1 << 40) + ra)


def test_wrappers_reject_bad_arguments():
    acc = softmax_sum((1, 8, 8, 19), 1)
    hist = torch.zeros((19, 16), dtype=torch.int64, device=DEV)
    bad_acc = [acc.double(), acc.permute(0, 3, 1, 2), acc[..., :1], acc.cpu(), acc[0]]
    for t in bad_acc:
        with pytest.raises(RuntimeError):
            F.confidence_histogram(t, hist)
    for h in (hist.int(), hist[:18], torch.zeros((19, 24), dtype=torch.int64, device=DEV),
              torch.zeros((19, 2048), dtype=torch.int64, device=DEV), hist.t().contiguous().t(), hist.cpu()):
        with pytest.raises(RuntimeError):
            F.confidence_histogram(acc, h)
    with pytest.raises(RuntimeError, match="pred"):
        F.confidence_histogram(acc, hist, pred=torch.zeros((1, 8, 8), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="cbin"):
        F.confidence_histogram(acc, hist, cbin=torch.zeros((1, 8, 8), dtype=torch.int16, device=DEV))
    with pytest.raises(RuntimeError, match="passes"):
        F.confidence_histogram(acc, hist, passes=0)
    with pytest.raises(RuntimeError, match="unsupported"):  # 32 x 1024 exceeds the LDS budget
        F.confidence_histogram(softmax_sum((1, 8, 8, 32), 1), torch.zeros((32, 1024), dtype=torch.int64, device=DEV))
    pred = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    cbin = _u16((1, 8, 8), 0)
    tbin = torch.zeros(19, dtype=torch.int32, device=DEV)
    for args in ((pred.long(), cbin, tbin), (pred, torch.zeros((1, 8, 8), dtype=torch.int32, device=DEV), tbin), (pred, cbin, tbin.long()),
                 (pred, cbin[:, :4], tbin), (pred, cbin, tbin.cpu()), (pred, cbin, tbin[:1])):
        with pytest.raises(RuntimeError):
            F.pseudo_select(*args, IGNORE)
    with pytest.raises(RuntimeError, match="out"):
        F.pseudo_select(pred, cbin, tbin, IGNORE, out=torch.zeros((1, 8, 8), dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0  # nothing was launched on the valid histogram


# ----------------------------------------------------------------------------- selection
@pytest.mark.parametrize("shape,bins", [((1, 13, 17, 19), 16), ((2, 24, 300, 19), 256), ((1, 16, 32, 32), 256),
                                        ((1, 8, 8, 2), 1024), (BIG, 1024)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pseudo_select_equals_where(shape, bins):
    c, ignore = shape[-1], 255  # (19 is a class of the 32-class shape)
    acc = softmax_sum(shape, 2, seed=21)
    hist, pred, cbin, (rh, rp, rb) = check(acc, bins, 2)
    rng = np.random.default_rng(4)
    populated = [int(np.nonzero(rh[k])[0][rng.integers(np.count_nonzero(rh[k]))]) if rh[k].any() else 0
                 for k in range(c)]
    tbins = [np.zeros(c, np.int32), np.full(c, bins, np.int32), np.array(populated, np.int32),
             rng.integers(0, bins + 1, c).astype(np.int32)]
    mixed = np.array(populated, np.int32)
    mixed[0], mixed[-1] = 0, bins
    tbins.append(mixed)
    out = torch.full(shape[:-1], -7, dtype=torch.int64, device=DEV)
    for tb in tbins:
        got = F.pseudo_select(pred, cbin, torch.from_numpy(tb).to(DEV), ignore, out=out)
        assert got is out
        want = np.where(rb >= tb[rp].astype(np.int64), rp, ignore)
        g = got.cpu().numpy()
        assert np.array_equal(g, want)
        for k in range(c):  # kept per class = the histogram's tail
            assert int((g == k).sum()) == int(rh[k, min(int(tb[k]), bins):].sum())
    # an unaligned view (pixel offset 3): the scalar path, and a fresh output
    pv, cv = pred.view(-1)[3:], cbin.view(-1)[3:]
    assert pv.is_contiguous() and pv.data_ptr() % 8 != 0
    got = F.pseudo_select(pv, cv, torch.from_numpy(tbins[2]).to(DEV), ignore)
    want = np.where(rb.reshape(-1)[3:] >= tbins[2][rp.reshape(-1)[3:]], rp.reshape(-1)[3:], ignore)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)


# ----------------------------------------------------------------------------- graph replay
def test_graph_capture_replay_equals_eager():
    shape, bins, passes = (2, 24, 300, 19), 1024, 2
    acc = softmax_sum(shape, passes, seed=31)
    rh, rp, rb = host_ref(acc, bins, passes)
    tbin = torch.from_numpy(np.random.default_rng(5).integers(0, bins, 19).astype(np.int32)).to(DEV)
    hist_e, pred_e, cbin_e = run_hist(acc, bins, passes)  # eager (and the first, warming call)
    lab_e = F.pseudo_select(pred_e, cbin_e, tbin, IGNORE)
    hist = torch.zeros((19, bins), dtype=torch.int64, device=DEV)
    pred = torch.zeros(shape[:-1], dtype=torch.uint8, device=DEV)
    cbin = _u16(shape[:-1], 0)
    lab = torch.zeros(shape[:-1], dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a straight line: two kernels on one stream
        F.confidence_histogram(acc, hist, passes=passes, pred=pred, cbin=cbin)
        F.pseudo_select(pred, cbin, tbin, IGNORE, out=lab)
    hist.zero_()
    pred.fill_(0xFF)
    lab.fill_(-1)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pred, pred_e) and np.array_equal(_np(cbin), _np(cbin_e)) and torch.equal(lab, lab_e)
    assert np.array_equal(_np(hist), 2 * rh) and np.array_equal(_np(hist_e), rh)


# ----------------------------------------------------------------------------- model level
SIZE, NB = (64, 128), 2


@pytest.fixture(scope="module")
def bisenet():
    net = BiSeNet(19, "resnet18")
    sd = net.state_dict()
    net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, 1))
    net = net.to(DEV).eval()
    batches = [(synthetic_images(2, *SIZE, seed=60 + i), torch.zeros(2, 1, *SIZE, dtype=torch.int64)) for i in range(NB)]
    return net, batches


def _generate_spied(monkeypatch, net, batches, **kw):
    """selftrain.generate with every predict_multiscale result (and its arguments) recorded."""
    seen = []
    real = validation.predict_multiscale

    def spy(model, inputs, size, scales, flip):
        acc, pred = real(model, inputs, size, scales, flip)
        seen.append((acc.clone(), tuple(size), tuple(scales), flip, inputs.cpu()))
        return acc, pred
    monkeypatch.setattr(selftrain, "predict_multiscale", spy)
    with rtsds_amd.precision(torch.float32):
        labels = selftrain.generate(net, batches, 19, device=DEV, **kw)
    torch.cuda.synchronize()
    return labels, seen


@pytest.mark.parametrize("scales,flip,bins", [((1.0,), False, 1024), ((0.75, 1.0), True, 256)])
def test_generate_equals_host_reference(bisenet, monkeypatch, scales, flip, bins):
    net, batches = bisenet
    labels, seen = _generate_spied(monkeypatch, net, batches, bins=bins, scales=scales, flip=flip)
    passes = len(scales) * (2 if flip else 1)
    assert len(labels) == NB == len(seen) and labels.bins == bins and not net.training
    total = np.zeros((19, bins), np.int64)
    for i, (acc, size, sc, fl, x) in enumerate(seen):
        assert size == SIZE and sc == tuple(scales) and fl == flip and torch.equal(x, batches[i][0])
        assert tuple(acc.shape) == (2, *SIZE, 19)
        rh, rp, rb = host_ref(acc, bins, passes)
        assert labels.pred[i].dtype == torch.uint8 and labels.cbin[i].dtype == torch.uint16
        assert np.array_equal(_np(labels.pred[i]), rp) and np.array_equal(_np(labels.cbin[i]), rb)
        total += rh
    assert np.array_equal(_np(labels.hist), total)


def test_thresholded_labels_and_one_training_epoch(bisenet, monkeypatch):
    net, batches = bisenet
    labels, _ = _generate_spied(monkeypatch, net, batches, store="cpu")
    assert not labels.pred[0].is_cuda
    tbin = selftrain.class_thresholds(labels.hist, 0.5)
    loader = selftrain.PseudoLabelLoader(batches, labels, tbin, IGNORE)
    assert len(loader) == NB
    h = _np(labels.hist)
    kept = np.zeros(19, np.int64)
    for i, (x, y) in enumerate(loader):
        assert x is batches[i][0] and y.dtype == torch.int64 and tuple(y.shape) == (2, 1, *SIZE) and y.is_cuda
        g = y.cpu().numpy()
        assert np.isin(g, np.arange(20)).all()                       # {0..18, 19}
        p = _np(labels.pred[i])
        assert ((g[:, 0] == p) | (g[:, 0] == IGNORE)).all()
        kept += np.bincount(g.reshape(-1), minlength=20)[:19]
    for k in range(19):
        assert kept[k] == h[k, min(int(tbin[k]), 1024):].sum()
        assert 2 * kept[k] >= h[k].sum()                             # at least half of each class
    frac = selftrain.kept_fraction(labels, tbin)
    assert all(np.isnan(f) or f >= 0.5 for f in frac) and kept.sum() > 0

    losses_seen = []

    class Log(Callback):
        def on_batch_end(self, batch, logs=None):
            losses_seen.append(logs["train_loss"])
    before = [p.detach().clone() for p in net.parameters()]
    opt = optim.Adam(net.parameters(), lr=1e-4)
    with rtsds_amd.precision(torch.float32):
        train.train(epoch=0, model=net, train_loader=loader, criterion=losses.CrossEntropyLoss(ignore_index=IGNORE),
                    optimizer=opt, init_lr=1e-4, max_iter=NB, device=DEV, callbacks=[Log()])
    torch.cuda.synchronize()
    net.eval()
    assert len(losses_seen) == NB and all(np.isfinite(v) and v > 0 for v in losses_seen)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    assert all(torch.isfinite(p).all() for p in net.parameters())


# ----------------------------------------------------------------------------- CLI
def _cfg(tmp_path, precision):
    cfg = yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))
    cfg["precision"] = precision
    cfg["data"]["cityscapes"].update(image_size="64, 128", batch_size=2)
    cfg["data"]["gta5_modified"].update(image_size="64, 128", batch_size=2)
    cfg["data"]["synthetic_batches"] = 2
    cfg["training"]["domain_adaptation"].update(iterations=2, epochs=1)
    cfg["training"]["segmentation"].update(epochs=1)
    cfg["model"]["adversarial_model"]["generator"]["name"] = "bisenet"
    cfg["training"]["self_training"] = {"rounds": 1, "epochs": 1, "portion": 0.2, "portion_step": 0.05, "cap": 0.9,
                                        "bins": 1024, "lr_scale": 0.1, "scales": [1.0], "flip": False}
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def _count_self_training(monkeypatch):
    calls = []
    real_gen, real_train = selftrain.generate, rmain.train
    monkeypatch.setattr(selftrain, "generate", lambda *a, **k: (calls.append("generate"), real_gen(*a, **k))[1])

    def counted(**kw):
        if isinstance(kw["train_loader"], selftrain.PseudoLabelLoader):
            calls.append("train")
        return real_train(**kw)
    monkeypatch.setattr(rmain, "train", counted)
    return calls


def test_main_self_training_domain_adaptation(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    calls = _count_self_training(monkeypatch)
    rmain.main(["--config", _cfg(tmp_path, "bf16"), "--domain_adaptation", "--self_training"])
    assert calls == ["generate", "train"]


def test_main_self_training_segmentation(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    calls = _count_self_training(monkeypatch)
    rmain.main(["--config", _cfg(tmp_path, "fp32"), "--model", "bisenet", "--self_training"])
    assert calls == ["generate", "train"]
