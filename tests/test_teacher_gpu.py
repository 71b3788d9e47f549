"""Online mean-teacher self-training on the device (rtsds_ema_step, rtsds_ema_many,
rtsds_upsample_pseudo, ema.EMATeacher, selftrain.TeacherLoader, main --self_training with
mode: online).

Every comparison in this file is EXACT: the EMA kernels against the numpy restatement
tests/teacher_ref.py (three separately rounded fp32 operations, round-to-nearest-even bf16), the
fused label kernel against the three-kernel chain it replaces, the teacher against a torch
restatement of three separate ops.  Outputs are pre-filled with sentinels and the buffers carry
guard values, so an element a kernel did not write -- or wrote next to its range -- shows."""
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from oracle.weights import recipe_state_dict, synthetic_images, synthetic_labels  # noqa: E402
from rtsds_amd import _lib, losses, optim, selftrain, train  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import main as rmain  # noqa: E402
from rtsds_amd.callbacks import Callback  # noqa: E402
from rtsds_amd.ema import EMATeacher  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402
from tests import teacher_ref as R  # noqa: E402

DEV = torch.device("cuda", 0)
GUARD = 12345.0


def _mixed(rng, n):
    """Values of mixed magnitude (1e-6 .. 1e6) and sign."""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32)


def _u16(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def _bins(cbin):
    """A uint16 bin map as an int32 device tensor."""
    return torch.from_numpy(_u16(cbin).astype(np.int32)).to(DEV)


# ----------------------------------------------------------------------------- rtsds_ema_step
@pytest.mark.parametrize("w", [0.0, 1.0, float(np.float32(0.01))])
@pytest.mark.parametrize("n", [1, 63, 197, 2 ** 20 + 3])  # the last: more than one pass of the 4096 x 256 grid
def test_ema_step_equals_reference(n, w):
    rng = np.random.default_rng(n)
    t0, s0 = _mixed(rng, n), _mixed(rng, n)
    want, want_bits = R.ema_ref(t0, s0, w)
    if w == 0.0:
        assert np.array_equal(want, t0)
    for off in (0, 1):  # off = 1: views one element into the allocation, the non-16-B path
        tbuf = torch.full((n + 9,), GUARD, dtype=torch.float32, device=DEV)
        sbuf = torch.full((n + 9,), GUARD, dtype=torch.float32, device=DEV)
        hbuf = torch.full((n + 9,), GUARD, dtype=torch.bfloat16, device=DEV)
        t, s, h = tbuf[off:off + n], sbuf[off:off + n], hbuf[off:off + n]
        assert (t.data_ptr() % 16 == 0) == (off == 0) and (h.data_ptr() % 16 == 0) == (off == 0)
        t.copy_(torch.from_numpy(t0))
        s.copy_(torch.from_numpy(s0))
        assert F.ema_step(t, s, w, h) is t
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), want), (n, w, off)
        assert np.array_equal(_u16(h), want_bits), (n, w, off)
        assert torch.equal(h, t.to(torch.bfloat16))
        assert np.array_equal(s.cpu().numpy(), s0)
        for buf in (tbuf, sbuf, hbuf):  # nothing next to the range was touched
            g = float(torch.tensor(GUARD).to(buf.dtype))
            assert (buf[:off].float() == g).all() and (buf[off + n:].float() == g).all()
    # without a shadow
    t = torch.from_numpy(t0).to(DEV)
    F.ema_step(t, torch.from_numpy(s0).to(DEV), w)
    assert np.array_equal(t.cpu().numpy(), want)


def test_ema_step_refusals():
    t, s = torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)
    for kw in ({"teacher": t.double()}, {"student": s[:8]}, {"student": s.cpu()}, {"shadow": torch.zeros(16, device=DEV)},
               {"teacher": torch.zeros(4, 4, device=DEV)}, {"teacher": torch.zeros(0, device=DEV)},
               {"student": torch.zeros(32, device=DEV)[::2]}):
        args = dict({"teacher": t, "student": s, "w": 0.5, "shadow": None}, **kw)
        with pytest.raises(RuntimeError, match="rtsds_amd: ema_step"):
            F.ema_step(**args)
    lib = _lib.load()
    assert lib.rtsds_ema_step(t.data_ptr(), s.data_ptr(), None, 0, 0.5, None) == 1
    assert lib.rtsds_ema_step(None, s.data_ptr(), None, 16, 0.5, None) == 2
    assert lib.rtsds_ema_step(t.data_ptr(), None, None, 16, 0.5, None) == 2
    assert lib.rtsds_ema_many(0, None, None, None, 0.5, None) == 1


# ----------------------------------------------------------------------------- rtsds_ema_many
def test_ema_many_equals_reference_and_leaves_neighbours_alone():
    sizes = [1, 19, 64, 128, 1000]
    rng = np.random.default_rng(7)
    w = float(np.float32(0.3))
    total = sum(sizes) + 3 * (len(sizes) + 1)
    tbuf = torch.full((total,), GUARD, dtype=torch.float32, device=DEV)
    sbuf = torch.full((total,), GUARD, dtype=torch.float32, device=DEV)
    pairs, want, pos = [], [], 3
    guard = torch.ones(total, dtype=torch.bool)
    for n in sizes:  # three guard elements before, between and after the segments
        t0, s0 = _mixed(rng, n), _mixed(rng, n)
        tbuf[pos:pos + n].copy_(torch.from_numpy(t0))
        sbuf[pos:pos + n].copy_(torch.from_numpy(s0))
        pairs.append((tbuf[pos:pos + n], sbuf[pos:pos + n]))
        want.append((R.ema_ref(t0, s0, w)[0], s0))
        guard[pos:pos + n] = False
        pos += n + 3
    table = F.EmaTable(pairs)
    assert table.count == 5 and not table.stale()
    F.ema_many(table, w)
    torch.cuda.synchronize()
    for (t, s), (tw, sw) in zip(pairs, want):
        assert np.array_equal(t.cpu().numpy(), tw) and np.array_equal(s.cpu().numpy(), sw)
    assert (tbuf.cpu()[guard] == GUARD).all() and (sbuf.cpu()[guard] == GUARD).all()
    # a moved tensor is noticed on the host
    moved = F.EmaTable([(torch.zeros(4, device=DEV), torch.zeros(4, device=DEV))])
    moved.pairs[0] = (torch.zeros(4, device=DEV), moved.pairs[0][1])
    assert moved.stale()
    with pytest.raises(RuntimeError, match="moved"):
        F.ema_many(moved, w)


# ----------------------------------------------------------------------------- rtsds_upsample_pseudo
IGNORE = 255


def _head(n, c, hi, wi, dtype, seed, gain=3.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, hi, wi, c, generator=g) * gain).to(dtype).to(DEV)
    return x.permute(0, 3, 1, 2)  # logical NCHW, NHWC memory


def _chain(x, geo, bins, tbin):
    """upsample_softmax_accumulate(accumulate=False) -> confidence_histogram(passes=1) -> pseudo_select."""
    n, c = x.shape[:2]
    ho, wo = geo[:2]
    acc = torch.empty((n, ho, wo, c), dtype=torch.float32, device=DEV)
    F.upsample_softmax_accumulate(x, geo, acc, accumulate=False)
    hist = torch.zeros((c, bins), dtype=torch.int64, device=DEV)
    pred = torch.empty((n, ho, wo), dtype=torch.uint8, device=DEV)
    cbin = torch.empty((n, ho, wo), dtype=torch.uint16, device=DEV)
    F.confidence_histogram(acc, hist, passes=1, pred=pred, cbin=cbin)
    return acc, pred, cbin, F.pseudo_select(pred, cbin, tbin, IGNORE)


def _sentinels(n, ho, wo):
    return (torch.full((n, ho, wo), 0xFF, dtype=torch.uint8, device=DEV),
            torch.full((n, ho, wo), -1, dtype=torch.int16, device=DEV).view(torch.uint16),
            torch.full((n, ho, wo), -7, dtype=torch.int64, device=DEV))


def _tbin(c, bins, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, bins // 2, (c,), generator=g, dtype=torch.int32)
    t[0], t[1] = bins, 0  # class 0 keeps nothing, class 1 keeps all
    return t.to(DEV)


def _check_against_chain(x, size, bins, seed=0):
    n, c = x.shape[:2]
    geo = F.upsample_geometry(x, size=size)
    tbin = _tbin(c, bins, seed)
    acc, pred_w, cbin_w, lab_w = _chain(x, geo, bins, tbin)
    pred, cbin, lab = _sentinels(n, *size)
    out = F.upsample_pseudo(x, geo, bins, tbin=tbin, ignore_index=IGNORE, pred=pred, cbin=cbin, labels=lab)
    assert out[0] is pred and out[1] is cbin and out[2] is lab
    torch.cuda.synchronize()
    assert torch.equal(pred, pred_w)
    assert np.array_equal(_u16(cbin), _u16(cbin_w))
    assert torch.equal(lab, lab_w)
    # outputs requested singly
    p1, c1, l1 = F.upsample_pseudo(x, geo, bins, tbin=tbin, ignore_index=IGNORE)
    assert p1 is None and c1 is None and torch.equal(l1, lab_w)
    p2, c2, l2 = F.upsample_pseudo(x, geo, bins)
    assert l2 is None and torch.equal(p2, pred_w) and np.array_equal(_u16(c2), _u16(cbin_w))
    # and the chain itself is what the numpy restatement says of its probabilities
    rp, rc, rl = R.pseudo_ref(acc.cpu().numpy(), bins, tbin.cpu().numpy(), IGNORE)
    assert np.array_equal(pred.cpu().numpy(), rp) and np.array_equal(_u16(cbin), rc)
    assert np.array_equal(lab.cpu().numpy(), rl)
    return pred, cbin, lab, tbin


CASES = {
    "c19_bf16_one_tile": (lambda: _head(2, 19, 5, 7, torch.bfloat16, 1), (40, 56), 1024),
    "c19_fp32_one_tile": (lambda: _head(2, 19, 5, 7, torch.float32, 2), (40, 56), 1024),
    "c19_two_tiles_ragged": (lambda: _head(1, 19, 3, 38, torch.bfloat16, 3), (6, 300), 1024),
    "c19_fp32_two_tiles_ragged": (lambda: _head(1, 19, 3, 38, torch.float32, 4), (6, 300), 256),
    "c5_runtime_count": (lambda: _head(2, 5, 4, 9, torch.bfloat16, 5), (9, 270), 16),
    "c32_runtime_count": (lambda: _head(1, 32, 4, 9, torch.float32, 6), (9, 270), 512),
    "c32_unstaged": (lambda: _head(1, 32, 2, 2048, torch.bfloat16, 7), (4, 64), 512),  # 2 x 2050 x 32 x 4 B > 64 KiB
    "c19_unstaged_fp32": (lambda: _head(1, 19, 2, 1024, torch.float32, 8), (3, 100), 1024),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_upsample_pseudo_equals_chain(name):
    make, size, bins = CASES[name]
    x = make()
    pred, cbin, lab, tbin = _check_against_chain(x, size, bins, seed=len(name))
    kept = lab != IGNORE
    assert kept.any() and (~kept).any()  # both arms of the threshold are exercised
    assert not (lab == 0).any()  # class 0: tbin = bins keeps nothing
    assert torch.equal(lab[pred == 1], torch.ones_like(lab[pred == 1]))  # class 1: tbin = 0 keeps all
    assert pred.unique().numel() > 2 and int(_bins(cbin).max()) < bins


def test_upsample_pseudo_nan_row_and_ties():
    x = _head(1, 19, 5, 7, torch.float32, 11).contiguous(memory_format=torch.channels_last)
    x[0, :, 2, 3] = float("nan")  # one low-resolution pixel: every output pixel that taps it is NaN
    pred, cbin, lab, tbin = _check_against_chain(x, (40, 56), 1024, seed=1)
    nan_px = (_bins(cbin) == 0) & (pred == 0)
    assert 0 < int(nan_px.sum()) < pred.numel() // 4  # the NaN rows: first NaN = class 0, bin 0
    assert (lab[nan_px] == IGNORE).all()
    y = _head(1, 19, 5, 7, torch.bfloat16, 12).contiguous(memory_format=torch.channels_last)
    y[:, 3] = 40.0
    y[:, 7] = 40.0  # two equal maxima everywhere: the first wins
    pred, cbin, lab, tbin = _check_against_chain(y, (40, 56), 1024, seed=2)
    assert (pred == 3).all()
    assert (_bins(cbin) == 511).all() or (_bins(cbin) == 512).all()  # conf ~ 0.5


def test_upsample_pseudo_refusals():
    x = _head(1, 19, 5, 7, torch.float32, 13)
    geo = F.upsample_geometry(x, size=(40, 56))
    tbin = _tbin(19, 1024, 0)
    lab = torch.empty((1, 40, 56), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="2..32 classes"):
        F.upsample_pseudo(x[:, :1], geo)  # c = 1
    with pytest.raises(RuntimeError, match="bins"):
        F.upsample_pseudo(x, geo, 48)
    with pytest.raises(RuntimeError, match="tbin"):
        F.upsample_pseudo(x, geo, labels=lab)  # labels without tbin
    for kw in ({"tbin": tbin[:5], "ignore_index": 1}, {"tbin": tbin.long(), "ignore_index": 1}, {"tbin": tbin},
               {"tbin": tbin.cpu(), "ignore_index": 1}, {"pred": torch.empty((1, 40, 56), dtype=torch.int8, device=DEV)},
               {"cbin": torch.empty((1, 40, 55), dtype=torch.uint16, device=DEV)},
               {"tbin": tbin, "ignore_index": 1, "labels": lab.int()}):
        with pytest.raises(RuntimeError, match="rtsds_amd: upsample_pseudo"):
            F.upsample_pseudo(x, geo, **kw)
    lib = _lib.load()
    xc = x.contiguous(memory_format=torch.channels_last)

    def raw(c=19, bins=1024, pred=None, cbin=None, tb=None, labels=None):
        return lib.rtsds_upsample_pseudo(xc.data_ptr(), pred, cbin, tb, labels, 1, 5, 7, c, 40, 56, geo[2], geo[3], bins,
                                         IGNORE, 0, None)
    assert raw(c=1, labels=lab.data_ptr(), tb=tbin.data_ptr()) == 1
    assert raw(bins=48, labels=lab.data_ptr(), tb=tbin.data_ptr()) == 1
    assert raw(labels=lab.data_ptr()) == 2  # labels without tbin
    assert raw() == 2                       # all outputs NULL
    assert raw(labels=lab.data_ptr() + 4, tb=tbin.data_ptr()) == 2  # misaligned labels
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- EMATeacher
SIZE = (64, 128)  # the smallest BiSeNet-R18 input of the model tests


def _net(seed):
    net = BiSeNet(19, "resnet18")
    sd = net.state_dict()
    net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed))
    return net.to(DEV)


def _steps(with_teacher):
    """Three seg_steps of BiSeNet-R18 on random labels (bf16 compute), update() after each."""
    net = _net(1).train()
    opt = optim.Adam(net.parameters(), lr=1e-3)
    crit = losses.CrossEntropyLoss(ignore_index=19)
    teacher = EMATeacher(net, _net(2), opt, decay=0.9) if with_teacher else None
    ema = {k: v.detach().clone() for k, v in net.state_dict().items()}
    out = []
    for i in range(3):
        x = synthetic_images(2, *SIZE, seed=80 + i).to(DEV)
        y = synthetic_labels(2, *SIZE, seed=90 + i).to(DEV)
        loss, _ = train.seg_step(net, crit, opt, x, y)
        out.append(loss.clone())
        if teacher is not None:
            w = teacher.weight()
            assert w == R.weight_ref(0.9, i)
            teacher.update()
            for k, cur in net.state_dict().items():
                if cur.is_floating_point():
                    d = cur - ema[k]
                    d = d * w
                    ema[k] = ema[k] + d
                else:
                    ema[k] = cur.detach().clone()
    torch.cuda.synchronize()
    snap = None if teacher is None else {k: v.detach().clone() for k, v in teacher.model.state_dict().items()}
    return net, opt, teacher, ema, out, snap


@pytest.fixture(scope="module")
def taught():
    with rtsds_amd.precision(torch.bfloat16):
        return _steps(True)


def test_teacher_state_equals_three_op_restatement(taught):
    net, opt, teacher, ema, _, sd = taught  # sd: the teacher's state_dict right after the three updates
    assert teacher.updates >= 3 and not teacher.model.training
    assert sd.keys() == ema.keys()
    moved = 0
    for k, v in sd.items():
        assert torch.equal(v, ema[k]), k
        moved += int(not torch.equal(v, net.state_dict()[k]))
    assert moved > len(sd) // 2  # the teacher lags the student: the comparison is not student == student
    assert all(not p.requires_grad for p in teacher.model.parameters())


def test_teacher_forward_uses_fresh_shadows_and_folds(taught):
    teacher = taught[2]
    x = synthetic_images(2, *SIZE, seed=99).to(DEV)
    with rtsds_amd.precision(torch.bfloat16), torch.no_grad():
        got = teacher.model(x)
        fresh = _net(3).eval()
        fresh.load_state_dict(teacher.model.state_dict())
        want = fresh(x)
        assert torch.equal(got, want)
        # one more update moves the teacher: the shadows and the BatchNorm folds follow
        teacher_sd = {k: v.clone() for k, v in teacher.state_dict()["model"].items()}
        updates = teacher.updates
        teacher.update()
        again = teacher.model(x)
        fresh.load_state_dict(teacher.model.state_dict())
        assert torch.equal(again, fresh(x)) and not torch.equal(again, got)
        # state_dict -> load_state_dict into a second teacher reproduces the forward
        state = teacher.state_dict()
        assert state["updates"] == updates + 1 and state["decay"] == 0.9 and set(state) == {"model", "updates", "decay"}
        other = EMATeacher(teacher.student, _net(4), teacher.optimizer, decay=0.5)
        other.load_state_dict(state)
        assert other.updates == updates + 1 and other.decay == 0.9
        assert torch.equal(other.model(x), again)
        # and the earlier state too
        other.load_state_dict({"model": teacher_sd, "updates": updates, "decay": 0.9})
        assert torch.equal(other.model(x), got)


def test_student_is_unaffected_by_the_teacher(taught):
    with rtsds_amd.precision(torch.bfloat16):
        alone = _steps(False)[4]
    with_teacher = taught[4]
    assert len(alone) == 3 and all(torch.isfinite(v).all() for v in alone)
    for a, b in zip(alone, with_teacher):
        assert torch.equal(a, b)


def test_teacher_refuses_parameter_outside_the_optimizer():
    student, teacher = torch.nn.Conv2d(3, 8, 3).to(DEV), torch.nn.Conv2d(3, 8, 3).to(DEV)
    opt = optim.Adam([student.weight], lr=1e-3)
    with pytest.raises(RuntimeError, match="parameter bias"):
        EMATeacher(student, teacher, opt)
    with pytest.raises(RuntimeError, match="do not match"):
        EMATeacher(student, torch.nn.Conv2d(3, 8, 3, bias=False).to(DEV), optim.Adam(student.parameters(), lr=1e-3))


def test_update_refuses_graph_capture(monkeypatch):
    student, teacher = torch.nn.Conv2d(3, 8, 3).to(DEV), torch.nn.Conv2d(3, 8, 3).to(DEV)
    t = EMATeacher(student, teacher, optim.Adam(student.parameters(), lr=1e-3))
    t.update()
    assert torch.equal(teacher.weight, student.weight) and torch.equal(teacher.bias, student.bias)  # w = 1, t == s
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        t.update()
    assert t.updates == 1


# ----------------------------------------------------------------------------- TeacherLoader
NB = 4


@pytest.fixture()
def loader_parts():
    net = _net(1).eval()
    batch0 = synthetic_images(2, *SIZE, seed=60).to(DEV)
    # the recipe weights saturate the softmax (every confidence in the top bin): scale the final
    # 1x1 classifier so that the logits have unit spread and the confidences cover many bins
    with torch.no_grad(), rtsds_amd.precision(torch.float32):
        (low, _), = net.forward_lowres(batch0, main_only=True)
        f = float(1.0 / low.float().std())
        net.conv.weight.mul_(f)
        net.conv.bias.mul_(f)
    net.train()
    opt = optim.Adam(net.parameters(), lr=1e-3)
    teacher = EMATeacher(net, _net(2), opt, decay=0.9)
    batches = [(synthetic_images(2, *SIZE, seed=60 + i), torch.zeros(2, 1, *SIZE, dtype=torch.int64)) for i in range(NB)]
    g = torch.Generator().manual_seed(9)
    ssize = (80, 160)
    source = [(synthetic_images(3, *ssize, seed=70 + i), torch.randint(0, 20, (3, 1, *ssize), generator=g))
              for i in range(3)]
    return net, opt, teacher, batches, source


def _head_of(teacher, x):
    with torch.no_grad():
        (low, _), = teacher.model.forward_lowres(x.to(DEV), main_only=True)
    return low, F.upsample_geometry(low, size=SIZE)


def _median_threshold(teacher, x, bins):
    low, geo = _head_of(teacher, x)
    _, cbin, _ = F.upsample_pseudo(low, geo, bins)
    b = _bins(cbin)
    assert b.unique().numel() > 8  # the confidences are spread: a threshold splits them
    return float(b.float().median()) / bins


def test_teacher_loader_labels_and_updates(loader_parts):
    net, opt, teacher, batches, _ = loader_parts
    crit = losses.CrossEntropyLoss(ignore_index=19)
    with rtsds_amd.precision(torch.float32):
        thr = _median_threshold(teacher, batches[0][0], 1024)
        loader = selftrain.TeacherLoader(batches, teacher, threshold=thr, ignore_index=19)
        assert len(loader) == NB and loader.tbin_value == R.tbin_ref(thr, 1024)
        tbin = torch.full((19,), loader.tbin_value, dtype=torch.int32, device=DEV)
        it = iter(loader)
        kept_total = 0
        for i in range(NB):
            x, y = next(it)
            assert teacher.updates == i  # the update of batch i - 1 ran when the iterator resumed, none since
            low, geo = _head_of(teacher, batches[i][0])  # the teacher is as it was just before the yield
            want = F.upsample_pseudo(low, geo, 1024, tbin=tbin, ignore_index=19)[2]
            assert x is batches[i][0]
            assert y.dtype == torch.int64 and tuple(y.shape) == (2, 1, *SIZE) and torch.equal(y[:, 0], want)
            kept = int((y != 19).sum())
            assert int(loader.last_kept) == kept
            if i == 0:
                assert 0 < kept < y.numel()  # the median threshold: both arms
            kept_total += kept
            train.seg_step(net, crit, opt, x.to(DEV), y[:, 0])  # the consumer's step on this batch
        with pytest.raises(StopIteration):
            next(it)
        assert teacher.updates == NB
        assert int(loader.kept_sum) == kept_total and loader.pixels == NB * 2 * SIZE[0] * SIZE[1]
        # a consumer that abandons the iterator skips the last update
        for _ in loader:
            break
        assert teacher.updates == NB


def test_teacher_loader_classmix_equals_functional(loader_parts):
    net, opt, teacher, batches, source = loader_parts
    with rtsds_amd.precision(torch.float32):
        thr = _median_threshold(teacher, batches[0][0], 1024)
        loader = selftrain.TeacherLoader(batches, teacher, threshold=thr, ignore_index=19, source_loader=source)
        tbin = torch.full((19,), loader.tbin_value, dtype=torch.int32, device=DEV)
        torch.manual_seed(123)
        it = iter(loader)
        for i in range(NB):
            before = torch.get_rng_state()
            x, y = next(it)
            after = torch.get_rng_state()
            low, geo = _head_of(teacher, batches[i][0])  # the teacher is as it was just before the yield
            pred, cbin, _ = F.upsample_pseudo(low, geo, 1024)
            torch.set_rng_state(before)  # the same draws, in ClassMixLoader's documented order
            blk = selftrain.ClassMixLoader.draw(2, 19, 80, 160, *SIZE).to(DEV)
            assert torch.equal(torch.get_rng_state(), after)
            simg, slab = source[i % 3]
            want_x, want_y = F.classmix(F.pack_input(simg[:2].to(DEV), torch.float32), slab[:2].to(DEV).long().contiguous(),
                                        F.pack_input(batches[i][0].to(DEV), torch.float32), pred, cbin, tbin,
                                        blk[:, 2:], blk[:, :2], 19)
            assert torch.equal(x, want_x) and torch.equal(y[:, 0], want_y)
            assert int(loader.last_kept) == int((y != 19).sum())
            assert (loader.last_chosen.cpu().view(torch.int32) != 0).all()  # every sample pasted some class
            assert x.is_cuda and tuple(x.shape) == (2, 3, *SIZE) and tuple(y.shape) == (2, 1, *SIZE)
        assert teacher.updates == NB - 1  # the last batch's update runs when the iterator is resumed
        with pytest.raises(StopIteration):
            next(it)
        assert teacher.updates == NB


# ----------------------------------------------------------------------------- CLI
def _cfg(tmp_path, precision, mix):
    cfg = yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))
    cfg["precision"] = precision
    cfg["data"]["cityscapes"].update(image_size="64, 128", batch_size=2)
    cfg["data"]["gta5_modified"].update(image_size="80, 160", batch_size=2)
    cfg["data"]["synthetic_batches"] = 2
    cfg["training"]["segmentation"].update(epochs=1)
    # 19 classes: the largest probability is at least 1 / 19 > 0.05, so every pixel is labelled
    cfg["training"]["self_training"] = {"mode": "online", "epochs": 1, "lr_scale": 0.1, "ema_decay": 0.99, "threshold": 0.05}
    if mix:
        cfg["training"]["self_training"]["mix"] = mix
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


@pytest.mark.parametrize("mix,precision", [(None, "bf16"), ("classmix", "fp32")])
def test_main_online_self_training(tmp_path, monkeypatch, mix, precision):
    monkeypatch.chdir(tmp_path)
    seen = {"teacher": None, "losses": []}
    real_self_train, real_train = rmain.self_train, rmain.train

    class Log(Callback):
        def on_batch_end(self, batch, logs=None):
            seen["losses"].append(logs["train_loss"])

    def counted(**kw):
        if isinstance(kw["train_loader"], selftrain.TeacherLoader):
            kw["callbacks"] = list(kw["callbacks"]) + [Log()]
            assert (kw["train_loader"].source_loader is not None) == (mix is not None)
        return real_train(**kw)

    def captured(*a, **k):
        seen["teacher"] = real_self_train(*a, **k)
        return seen["teacher"]
    monkeypatch.setattr(rmain, "train", counted)
    monkeypatch.setattr(rmain, "self_train", captured)
    monkeypatch.setattr(selftrain, "generate", lambda *a, **k: pytest.fail("the offline sweep ran in online mode"))
    before = rtsds_amd.compute_dtype()
    try:
        rmain.main(["--config", _cfg(tmp_path, precision, mix), "--model", "bisenet", "--self_training"])
    finally:
        rtsds_amd.set_compute_dtype(before)
    assert isinstance(seen["teacher"], EMATeacher) and seen["teacher"].updates == 2  # two iterations
    assert len(seen["losses"]) == 2 and all(np.isfinite(v) and v > 0 for v in seen["losses"])
