"""Knowledge distillation on the device (csrc/distill.hip, functional.distill_kl, rtsds_amd.distill,
main --distill) against the fp64 statement of tests/distill_ref.py.  Tolerances: 8 x max(error of the
fp32 numpy restatement of the kernel's formulas on the same inputs, one fp32 ulp of the reference
value) for the loss and for the gradient at its largest element (tests/pinned/distill_tol.json; the
margin covers a summation order other than numpy's and the hardware's expf / logf), plus 2^-8 |ref|
per element of a bf16 gradient (its rounding and one boundary flip).  The premises -- the fp64
statement is torch's, no resampled row has a near-tie, so `agree` is exact -- are checked in
tests/test_distill_cpu.py.

Shapes (n, c, hs, ws <- ht, wt), each in fp32 and bf16, T in {0.5, 1, 4} taking turns:
(2,19, 8,16 <- 9,17) DeepLab -> BiSeNet at a 64x128 input: the c = 19 instantiation, a slight
downsample, the image stride; (1,19, 13,17 <- 13,17) identity taps, odd sizes; (2,7, 9,40 <- 5,21)
runtime c, a non-integer upsample; (1,32, 4,4 <- 7,3) the largest c, down in H and up in W;
(1,2, 4,4 <- 2,2) the smallest c; (1,19, 3,300 <- 5,77) a row of three tiles, the last a tail;
(1,19, 2,260 <- 2,4200) a source span too wide for the LDS: taps read from memory;
(1,19, 64,128 <- 65,129) the real geometry, at every T; (1,5, 2,3 <- 3,2000) runtime c on the
unstaged route (the host plan has two branches -- c == 19 or not, span staged or not -- and this
crosses them); one fp32-student / bf16-teacher pair."""
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from oracle.weights import recipe_state_dict, synthetic_images, synthetic_labels  # noqa: E402
from rtsds_amd import distill, losses, optim, train  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import main as rmain  # noqa: E402
from rtsds_amd._lib import lib  # noqa: E402
from rtsds_amd.callbacks import Callback  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402
from rtsds_amd.models.deeplabv2.deeplabv2 import get_deeplab_v2  # noqa: E402

from tests import distill_ref as R  # noqa: E402

DEV = torch.device("cuda", 0)
PINNED = R.pinned()
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 64      # bytes on either side of every output
SENTINEL = 0xA5


# ------------------------------------------------------------------ buffers
def _nhwc(a, dtype, offset=0):
    """The NHWC numpy array as a device tensor of logical shape [n, c, h, w] (channels_last memory);
    ``offset``: its base that many elements past an aligned allocation."""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(DEV).to(TORCH[dtype])
    buf = torch.zeros(flat.numel() + offset + 8, dtype=TORCH[dtype], device=DEV)
    buf[offset:offset + flat.numel()] = flat
    view = buf[offset:offset + flat.numel()].view(a.shape).permute(0, 3, 1, 2)
    assert view.data_ptr() % 16 == (offset * buf.element_size()) % 16 and view.is_contiguous(memory_format=torch.channels_last)
    return view


class Guarded:
    """``nbytes`` of output between two guards of sentinel bytes; ``offset`` bytes past 16-B alignment."""

    def __init__(self, nbytes, offset=0):
        self.raw = torch.full((nbytes + 2 * GUARD + offset,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.lo, self.hi = GUARD + offset, GUARD + offset + nbytes
        self.ptr = self.raw.data_ptr() + self.lo
        assert self.raw.data_ptr() % 16 == 0

    def view(self, dtype):
        return self.raw[self.lo:self.hi].view(dtype)

    def intact(self):
        return bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.hi:] == SENTINEL).all())


def run_entries(case, g=1.0, offset=0, want=True):
    """The three entries on guarded buffers: (loss, dx [n, hs, ws, c] as fp64 numpy or None, agree, raw
    results for bit comparisons).  ``offset``: inputs and dx one element past an aligned base."""
    (n, c, hs, ws, ht, wt), temp, sd, td = case
    cs = R.case(*case)
    s, t = _nhwc(cs.s, sd, offset), _nhwc(cs.t, td, offset)
    esz = s.element_size()
    nbytes = lib.rtsds_distill_workspace(n, hs, ws, c, ht, wt)
    assert nbytes > 0
    wsp, loss, agree = Guarded(nbytes), Guarded(4), Guarded(8)
    dx = Guarded(n * hs * ws * c * esz, offset * esz)
    agree.view(torch.int64).zero_()
    gt = torch.full((1,), g, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    pixels = float(n * hs * ws)
    lib.rtsds_distill_fwd(s.data_ptr(), F.dcode(s), t.data_ptr(), F.dcode(t), n, hs, ws, c, ht, wt, F._src_scale(ht, hs, None),
                          F._src_scale(wt, ws, None), float(np.float32(1.0 / temp)), int(want), agree.ptr, wsp.ptr, nbytes, st)
    lib.rtsds_distill_finish(wsp.ptr, nbytes, n, hs, ws, temp * temp / pixels, loss.ptr, st)
    if want:
        lib.rtsds_distill_bwd(wsp.ptr, nbytes, gt.data_ptr(), temp / pixels, dx.ptr, F.dcode(s), n, hs, ws, c, st)
    torch.cuda.synchronize()
    assert wsp.intact() and loss.intact() and agree.intact() and dx.intact()
    dxt = dx.view(TORCH[sd]).clone()
    if not want:
        assert bool((dx.view(torch.uint8) == SENTINEL).all())          # nothing was written
    return (float(loss.view(torch.float32)[0]), dxt.double().cpu().numpy().reshape(n, hs, ws, c) if want else None,
            int(agree.view(torch.int64)[0]), (loss.view(torch.float32).clone(), dxt))


def check(case, loss, dx, g=1.0):
    cs, p = R.case(*case), PINNED[R.key(*case)]
    ref = g * cs.grad64
    e_loss, e_grad = abs(loss - cs.loss64), np.abs(dx - ref)
    tol_loss = R.MARGIN * p["loss"]
    tol_grad = g * R.MARGIN * p["grad"] + (R.BF16_OUT * np.abs(ref) if case[2] == "bf16" else 0.0)
    print(f"{R.key(*case)} g={g}: loss {loss!r} (fp64 {cs.loss64!r}) off by {e_loss:.3e}, tolerance {tol_loss:.3e}; gradient off by "
          f"{e_grad.max():.3e} at most, {(e_grad / tol_grad).max():.3f} of its tolerance (max |gradient| {np.abs(ref).max():.3e})")
    assert e_loss <= tol_loss
    assert (e_grad <= tol_grad).all()


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_loss_gradient_and_agreement_against_fp64(case):
    loss, dx, agree, _ = run_entries(case)
    print(f"{R.key(*case)}: agree {agree}, fp64 {R.case(*case).agree}")
    check(case, loss, dx)
    assert agree == R.case(*case).agree


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[1], R.CASES[5], R.CASES[11]], ids=lambda c: R.key(*c))
def test_bases_one_element_past_an_aligned_allocation_give_the_same_bits(case):
    loss, dx, agree, raw = run_entries(case, offset=1)
    check(case, loss, dx)
    _, _, agree0, raw0 = run_entries(case)
    assert agree == agree0 == R.case(*case).agree
    assert torch.equal(raw[0], raw0[0]) and torch.equal(raw[1], raw0[1])


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[13], R.CASES[15]], ids=lambda c: R.key(*c))
def test_two_runs_give_equal_bits(case):
    a, b = run_entries(case), run_entries(case)
    assert torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1]) and a[2] == b[2]


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[5], R.CASES[11], R.CASES[15]], ids=lambda c: R.key(*c))
def test_an_upstream_gradient_of_a_quarter_scales_the_gradient(case):
    loss, dx, _, raw = run_entries(case, g=0.25)
    check(case, loss, dx, g=0.25)
    _, _, _, full = run_entries(case)
    assert torch.equal(raw[1].float() * 4.0, full[1].float())            # a power of two: the same bits, shifted


def test_forward_without_gradient_leaves_the_loss_and_writes_no_residual():
    case = R.CASES[0]
    loss, _, agree, raw = run_entries(case, want=False)
    full = run_entries(case)
    assert torch.equal(raw[0], full[3][0]) and agree == full[2]


# ------------------------------------------------------------------ the autograd function
def _fn(case, **kw):
    cs = R.case(*case)
    s = _nhwc(cs.s, case[2]).requires_grad_()
    t = _nhwc(cs.t, case[3])
    return s, t, F.distill_kl(s, t, case[1], **kw)


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[5], R.CASES[12], R.CASES[-1]], ids=lambda c: R.key(*c))
def test_function_equals_the_entries_and_the_teacher_gets_no_gradient(case):
    n, c, hs, ws, _, _ = case[0]
    agree = torch.zeros(1, dtype=torch.int64, device=DEV)
    s, t, loss = _fn(case, agree=agree)
    t.requires_grad_()
    loss2 = F.distill_kl(s, t, case[1])
    (loss + loss2).backward()
    _, _, agree_e, raw = run_entries(case, g=2.0)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and torch.equal(loss.detach(), raw[0][0]) and torch.equal(loss, loss2)
    assert s.grad.dtype == s.dtype and s.grad.shape == s.shape and t.grad is None
    assert torch.equal(s.grad.permute(0, 2, 3, 1).reshape(-1), raw[1])   # two equal terms = an upstream gradient of 2
    assert int(agree) == agree_e
    # NCHW memory gives the same result
    s2 = s.detach().contiguous().requires_grad_()
    l3 = losses.DistillationLoss(case[1])(s2, t.detach().contiguous())
    l3.backward()
    assert torch.equal(l3.detach(), loss.detach()) and torch.equal(s2.grad * 2, s.grad)


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[3], R.CASES[4], R.CASES[6], R.CASES[7], R.CASES[8], R.CASES[11], R.CASES[15]],
                         ids=lambda c: R.key(*c))
def test_teacher_equal_to_the_student_gives_exactly_zero(case):
    n, c, hs, ws, _, _ = case[0]
    cs = R.case(*case)
    s = _nhwc(cs.s, case[2]).requires_grad_()
    agree = torch.zeros(1, dtype=torch.int64, device=DEV)
    loss = F.distill_kl(s, s.detach().clone(), case[1], agree)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not bool(s.grad.any()) and int(agree) == n * hs * ws


def test_refusals():
    s = torch.zeros((2, 19, 4, 4), device=DEV)
    with pytest.raises(RuntimeError, match="classes"):
        F.distill_kl(s, torch.zeros((2, 7, 4, 4), device=DEV))
    with pytest.raises(RuntimeError, match=r"\[2, 32\]"):
        F.distill_kl(torch.zeros((2, 33, 4, 4), device=DEV), torch.zeros((2, 33, 4, 4), device=DEV))
    with pytest.raises(RuntimeError, match=r"\[2, 32\]"):
        F.distill_kl(torch.zeros((2, 1, 4, 4), device=DEV), torch.zeros((2, 1, 4, 4), device=DEV))
    with pytest.raises(RuntimeError, match="batch"):
        F.distill_kl(s, torch.zeros((3, 19, 4, 4), device=DEV))
    for temp in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="temperature"):
            F.distill_kl(s, s, temp)
    with pytest.raises(RuntimeError, match="HIP"):
        F.distill_kl(s, s.cpu())
    with pytest.raises(RuntimeError, match="HIP"):
        F.distill_kl(s, s, 1.0, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="agree"):
        F.distill_kl(s, s, 1.0, torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="dtype"):
        F.distill_kl(s.half(), s.half())
    with pytest.raises(RuntimeError, match=r"\[n, c, h, w\]"):
        F.distill_kl(s[0], s[0])


def test_graph_capture_of_forward_and_backward_replays_on_refreshed_inputs():
    shape, temp = R.SHAPES[0], 4.0
    n, c, hs, ws, ht, wt = shape
    s = torch.zeros((n, c, hs, ws), device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    t = torch.zeros((n, c, ht, wt), dtype=torch.bfloat16, device=DEV).contiguous(memory_format=torch.channels_last)
    agree = torch.zeros(1, dtype=torch.int64, device=DEV)
    (F.distill_kl(s, t, temp, agree) * 1.0).backward()                     # eager (and the first, warming call)
    s.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a straight line on one stream: forward, finish, backward
        loss = F.distill_kl(s, t, temp, agree)
        dx, = torch.autograd.grad(loss, s)
    for seed in (71, 72):
        sn, tn = R.logits((n, hs, ws, c), seed, "f32"), R.logits((n, ht, wt, c), seed + 10, "bf16")
        with torch.no_grad():
            s.copy_(_nhwc(sn, "f32"))
            t.copy_(_nhwc(tn, "bf16"))
        agree.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = (loss.detach().clone(), dx.clone(), int(agree))
        e_agree = torch.zeros(1, dtype=torch.int64, device=DEV)
        se = s.detach().clone().requires_grad_()
        le = F.distill_kl(se, t, temp, e_agree)
        le.backward()
        assert torch.equal(got[0], le.detach()) and torch.equal(got[1], se.grad) and got[2] == int(e_agree)
        want = R.distill(sn, tn, temp)
        assert abs(float(got[0]) - float(want[0])) <= 1e-5 * float(want[0]) and got[2] == want[2]


# ------------------------------------------------------------------ distill_step
SIZE = (64, 128)  # the smallest BiSeNet-R18 input of the model tests: heads 8x16, DeepLab's 9x17


def _load(net, seed):
    sd = net.state_dict()
    net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed))
    return net.to(DEV)


def _student(seed=1):
    return _load(BiSeNet(19, "resnet18"), seed).train()


def _teacher(kind):
    return _load(BiSeNet(19, "resnet18"), 2) if kind == "bisenet" else _load(get_deeplab_v2(19, pretrain=False), 3)


def _batch():
    return synthetic_images(2, *SIZE, seed=80).to(DEV), synthetic_labels(2, *SIZE, seed=90).to(DEV)


def _state(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kind,precision", [("bisenet", torch.float32), ("deeplab", torch.bfloat16)])
def test_distill_step(kind, precision):
    x, y = _batch()
    crit = losses.CrossEntropyLoss(ignore_index=19)
    with rtsds_amd.precision(precision):
        d = distill.Distiller(_teacher(kind).train(), temperature=2.0, weight=0.5)
        assert not d.teacher.training and not any(p.requires_grad for p in d.teacher.parameters())
        frozen = _state(d.teacher)
        net = _student()
        before = _state(net)
        # the same heads from a twin of the student (train-mode forward, same parameters)
        heads = _student().forward_lowres(x)
        thead = d.teacher_head(x)
        assert tuple(thead.shape[2:]) == ((8, 16) if kind == "bisenet" else (9, 17)) and not thead.requires_grad
        e_agree = torch.zeros(1, dtype=torch.int64, device=DEV)
        kd_ref = F.distill_kl(heads[0][0].detach(), thead, 2.0, e_agree)
        loss, correct, kd, agree = distill.distill_step(net, d, crit, optim.Adam(net.parameters(), lr=1e-3), x, y)
        torch.cuda.synchronize()
    assert _same(frozen, _state(d.teacher)) and not d.teacher.training     # parameters and BatchNorm buffers, bit for bit
    after = _state(net)
    assert any(not torch.equal(before[k], after[k]) for k, p in net.named_parameters())
    assert torch.equal(kd, kd_ref) and int(agree) == int(e_agree) and 0 <= int(agree) <= 2 * 8 * 16 == d.low_pixels
    assert np.isfinite(float(loss)) and float(kd) > 0 and 0 <= int(correct) <= 2 * 64 * 128
    print(f"{kind}: loss {float(loss):.4f}, kd {float(kd):.4f}, agree {int(agree)} of 256")


@pytest.mark.parametrize("precision", [torch.float32, torch.bfloat16])
def test_weight_zero_is_seg_step(precision):
    x, y = _batch()
    crit = losses.CrossEntropyLoss(ignore_index=19)

    def seg():
        net = _student()
        loss, correct = train.seg_step(net, crit, optim.Adam(net.parameters(), lr=1e-3), x, y)
        return _state(net), loss, correct

    with rtsds_amd.precision(precision):
        (a, la, ca), (b, lb, cb) = seg(), seg()
        assert _same(a, b) and torch.equal(la, lb) and torch.equal(ca, cb)        # the premise: seg_step repeats itself
        net = _student()
        d = distill.Distiller(_teacher("bisenet"), temperature=1.0, weight=0.0)
        loss, correct, kd, _ = distill.distill_step(net, d, crit, optim.Adam(net.parameters(), lr=1e-3), x, y)
        torch.cuda.synchronize()
    assert _same(a, _state(net)) and torch.equal(correct, ca) and float(kd) > 0
    assert torch.equal(loss, la)


def test_distill_step_refuses_a_student_without_lowres_heads():
    d = distill.Distiller(_teacher("bisenet"))
    net = torch.nn.Conv2d(3, 19, 1).to(DEV)
    x, y = _batch()
    with pytest.raises(RuntimeError, match="forward_lowres"):
        distill.distill_step(net, d, losses.CrossEntropyLoss(ignore_index=19), optim.Adam(net.parameters(), lr=1e-3), x, y)


# ------------------------------------------------------------------ main --distill
def _cfg(tmp_path, precision, teacher_model, weights):
    cfg = yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))
    cfg["precision"] = precision
    cfg["data"]["cityscapes"].update(image_size="64, 128", batch_size=2)
    cfg["data"]["gta5_modified"].update(image_size="80, 160", batch_size=2)
    cfg["data"]["synthetic_batches"] = 2
    cfg["training"]["segmentation"].update(epochs=1)
    cfg["training"]["distillation"] = {"teacher_model": teacher_model, "teacher_weights": weights, "temperature": 2.0, "weight": 0.5}
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


@pytest.mark.parametrize("teacher_model,precision", [("deeplab", "fp32"), ("bisenet", "bf16")])
def test_main_distill(tmp_path, monkeypatch, teacher_model, precision):
    monkeypatch.chdir(tmp_path)
    weights = str(tmp_path / "teacher.pth")
    torch.save({k: v.cpu() for k, v in _teacher(teacher_model).state_dict().items()}, weights)
    seen = {"logs": [], "distiller": None}
    real_train = distill.train

    class Log(Callback):
        def on_batch_end(self, batch, logs=None):
            seen["logs"].append(dict(logs))

    def logged(**kw):
        seen["distiller"] = kw["distiller"]
        kw["callbacks"] = list(kw["callbacks"]) + [Log()]
        return real_train(**kw)
    monkeypatch.setattr(distill, "train", logged)
    monkeypatch.setattr(rmain, "train", lambda **kw: pytest.fail("the plain loop ran under --distill"))
    before = rtsds_amd.compute_dtype()
    try:
        rmain.main(["--config", _cfg(tmp_path, precision, teacher_model, weights), "--model", "bisenet", "--distill"])
    finally:
        rtsds_amd.set_compute_dtype(before)
    d = seen["distiller"]
    assert isinstance(d, distill.Distiller) and (d.temperature, d.weight) == (2.0, 0.5) and not d.teacher.training
    assert isinstance(d.teacher, BiSeNet) == (teacher_model == "bisenet") and next(d.teacher.parameters()).is_cuda
    assert len(seen["logs"]) == 2                                               # two iterations
    for logs in seen["logs"]:
        assert np.isfinite(logs["distill_loss"]) and logs["distill_loss"] > 0
        assert 0.0 <= logs["teacher_agreement"] <= 100.0
        assert np.isfinite(logs["train_loss"]) and 0.0 <= logs["train_accuracy"] <= 100.0
