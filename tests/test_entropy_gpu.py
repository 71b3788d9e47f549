"""Target entropy minimisation on the device (csrc/entropy.hip, functional.entropy_loss,
rtsds_amd.entmin, main --entropy_min) against the fp64 statement of tests/entropy_ref.py.
Tolerances: 8 x max(error of the fp32 numpy restatement of the kernel's formulas on the same inputs,
one fp32 ulp of the reference value) for the loss, the mean entropy, the gradient at its largest
element and the map of h at its largest element (tests/pinned/entropy_tol.json; the margin covers a
summation order other than numpy's and the hardware's expf / logf / powf), plus 2^-8 |ref| per
element of a bf16 gradient (its rounding and one boundary flip).  The premise -- the fp64 statement
is torch's -- is checked in tests/test_entropy_cpu.py.

Shapes (n, c, h, w), each in fp32 and bf16, the penalties taking turns (robust with eta 2 and 0.5):
(2,19,8,16) two full tiles, the c = 19 instantiation; (1,19,13,17) a tail tile, odd sizes;
(2,7,9,40) runtime c, tiles crossing the image boundary; (1,2,4,4) and (1,32,4,4) the class-count
limits; (1,19,1,1) one pixel; (1,19,64,128) the real geometry, under every penalty."""
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from oracle.weights import recipe_state_dict, synthetic_images, synthetic_labels  # noqa: E402
from rtsds_amd import entmin, losses, optim, train  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import main as rmain  # noqa: E402
from rtsds_amd._lib import lib  # noqa: E402
from rtsds_amd.callbacks import Callback  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402
from rtsds_amd.models.deeplabv2.deeplabv2 import get_deeplab_v2  # noqa: E402

from tests import entropy_ref as R  # noqa: E402

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
    assert view.data_ptr() % 16 == (offset * buf.element_size()) % 16
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


def run_entries(x_np, dtype, penalty, eta, g=1.0, offset=0, want=True, world=1):
    """The three entries on guarded buffers, NHWC ``x_np``: a dict of loss, entropy (floats), dx
    [n, h, w, c] and map [n, h, w] as fp64 numpy (dx None without ``want``), and ``raw`` device
    results for bit comparisons.  ``offset``: input and dx one element past an aligned base."""
    n, h, w, c = x_np.shape
    x = _nhwc(x_np, dtype, offset)
    esz = x.element_size()
    nbytes = lib.rtsds_entropy_workspace(n, h, w, c)
    assert nbytes > 0
    wsp, loss, ment, hmap = Guarded(nbytes), Guarded(4), Guarded(4), Guarded(n * h * w * 4)
    dx = Guarded(n * h * w * c * esz, offset * esz)
    gt = torch.full((1,), g, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    coef = 1.0 / float(n * h * w * world)
    lib.rtsds_entropy_fwd(x.data_ptr(), F.dcode(x), n, h, w, c, F.ENTROPY_PENALTIES[penalty], float(np.float32(eta)), int(want),
                          hmap.ptr, wsp.ptr, nbytes, st)
    lib.rtsds_entropy_finish(wsp.ptr, nbytes, n, h, w, coef, loss.ptr, ment.ptr, st)
    if want:
        lib.rtsds_entropy_bwd(wsp.ptr, nbytes, gt.data_ptr(), coef, dx.ptr, F.dcode(x), n, h, w, c, st)
    torch.cuda.synchronize()
    assert wsp.intact() and loss.intact() and ment.intact() and hmap.intact() and dx.intact()
    dxt = dx.view(TORCH[dtype]).clone()
    part = ((-(-n * h * w // 128)) * 8 + 15) // 16 * 16
    if not want:   # nothing was written: neither dx nor the gradient term behind the partials
        assert bool((dx.view(torch.uint8) == SENTINEL).all()) and bool((wsp.view(torch.uint8)[part:] == SENTINEL).all())
    raw = (loss.view(torch.float32).clone(), ment.view(torch.float32).clone(), dxt, hmap.view(torch.float32).clone())
    return dict(loss=float(raw[0][0]), entropy=float(raw[1][0]), raw=raw,
                dx=dxt.double().cpu().numpy().reshape(n, h, w, c) if want else None,
                map=raw[3].double().cpu().numpy().reshape(n, h, w))


def run_case(case, **kw):
    return run_entries(R.case(*case).x, case[3], case[1], case[2], **kw)


def check(case, got, g=1.0):
    cs, p = R.case(*case), PINNED[R.key(*case)]
    ref = g * cs.grad64
    e_loss, e_ent = abs(got["loss"] - cs.loss64), abs(got["entropy"] - cs.ent64)
    e_grad, e_map = np.abs(got["dx"] - ref), np.abs(got["map"] - cs.map64)
    tol_grad = g * R.MARGIN * p["grad"] + (R.BF16_OUT * np.abs(ref) if case[3] == "bf16" else 0.0)
    print(f"{R.key(*case)} g={g}: loss {got['loss']!r} (fp64 {cs.loss64!r}) off by {e_loss:.3e}, tolerance {R.MARGIN * p['loss']:.3e}; "
          f"entropy {got['entropy']!r} (fp64 {cs.ent64!r}) off by {e_ent:.3e}, tolerance {R.MARGIN * p['entropy']:.3e}; "
          f"gradient off by {e_grad.max():.3e} at most, {(e_grad / tol_grad).max():.3f} of its tolerance (max |gradient| "
          f"{np.abs(ref).max():.3e}); map off by {e_map.max():.3e}, tolerance {R.MARGIN * p['map']:.3e}")
    assert e_loss <= R.MARGIN * p["loss"]
    assert e_ent <= R.MARGIN * p["entropy"]
    assert (e_grad <= tol_grad).all()
    assert (e_map <= R.MARGIN * p["map"]).all()


def same_bits(a, b, which=(0, 1, 2, 3)):
    return all(torch.equal(a["raw"][i], b["raw"][i]) for i in which)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_loss_entropy_gradient_and_map_against_fp64(case):
    check(case, run_case(case))


@pytest.mark.parametrize("penalty,eta", R.PENALTIES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_special_rows(penalty, eta, dtype):
    x = R.special_rows()
    got = run_entries(x, dtype, penalty, eta)
    want = R.entropy(x, penalty, eta)
    tol = R.MARGIN * 2.0 ** -23       # quantities of order one, a few fp32 roundings each
    dx, h = got["dx"], got["map"]
    print(f"{penalty} {eta} {dtype}: h {h.ravel()}, fp64 {want[3].ravel()}; loss {got['loss']!r}, fp64 {float(want[0])!r}; "
          f"constant row: max |dx| {np.abs(dx[0, 0, 1]).max():.3e}")
    assert np.isfinite(got["loss"]) and np.isfinite(got["entropy"]) and np.isfinite(dx).all() and np.isfinite(h).all()
    assert abs(got["loss"] - float(want[0])) <= tol and abs(got["entropy"] - float(want[1])) <= tol
    assert np.abs(h - want[3]).max() <= tol
    # the gradient carries 1 / (n h w) = 1 / 4
    assert np.abs(dx - want[2]).max() <= tol / 4 + (R.BF16_OUT * np.abs(want[2]).max() if dtype == "bf16" else 0.0)
    assert h[0, 0, 0] == 0.0 and not dx[0, 0, 0].any()                      # one logit at 200: exactly 0
    assert abs(h[0, 0, 1] - 1.0) <= tol and h[0, 0, 1] <= 1.0 and np.abs(dx[0, 0, 1]).max() <= tol   # a constant row
    assert not dx[0, 0, 2, [1, 4, 18]].any() and dx[0, 0, 2].any()          # classes at -inf
    assert dx[0, 0, 3, 2] == dx[0, 0, 3, 9]                                 # two equal maxima


# ------------------------------------------------------------------ bit stability
# a bf16 case, an fp32 case, the tail case, the real geometry
@pytest.mark.parametrize("case", [R.CASES[1], R.CASES[4], R.CASES[2], R.CASES[3], R.CASES[12], R.CASES[15]], ids=lambda c: R.key(*c))
def test_a_base_one_element_past_an_aligned_allocation_gives_the_same_bits(case):
    got = run_case(case, offset=1)
    check(case, got)
    assert same_bits(got, run_case(case))


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[5], R.CASES[13], R.CASES[16]], ids=lambda c: R.key(*c))
def test_two_runs_give_equal_bits(case):
    assert same_bits(run_case(case), run_case(case))


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[3], R.CASES[7], R.CASES[14]], ids=lambda c: R.key(*c))
def test_an_upstream_gradient_of_a_quarter_scales_the_gradient(case):
    got = run_case(case, g=0.25)
    check(case, got, g=0.25)
    full = run_case(case)
    assert torch.equal(got["raw"][2].float() * 4.0, full["raw"][2].float())   # a power of two: the same bits, shifted
    assert same_bits(got, full, (0, 1, 3))


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[3], R.CASES[15]], ids=lambda c: R.key(*c))
def test_forward_without_gradient_leaves_the_loss_and_writes_no_term(case):
    assert same_bits(run_case(case, want=False), run_case(case), (0, 1, 3))


# ------------------------------------------------------------------ the autograd function
def _fn(case, **kw):
    x = _nhwc(R.case(*case).x, case[3]).requires_grad_()
    return x, F.entropy_loss(x, case[1], case[2], **kw)


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[3], R.CASES[5], R.CASES[7], R.CASES[15]], ids=lambda c: R.key(*c))
def test_function_equals_the_entries_and_the_entropy_carries_no_gradient(case):
    n, c, h, w = case[0]
    hmap = torch.full((n, h, w), -1.0, device=DEV)
    x, (loss, ment) = _fn(case, entropy_map=hmap)
    loss2, ment2 = F.entropy_loss(x, case[1], case[2])
    assert not ment.requires_grad and ment.grad_fn is None and loss.requires_grad
    (loss + loss2).backward()
    e = run_case(case, g=2.0)
    for t, raw in ((loss, e["raw"][0]), (ment, e["raw"][1])):
        assert t.dtype == torch.float32 and t.dim() == 0 and torch.equal(t.detach(), raw[0])
    assert torch.equal(loss, loss2) and torch.equal(ment, ment2)
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    assert torch.equal(x.grad.permute(0, 2, 3, 1).reshape(-1), e["raw"][2])     # two equal terms = an upstream gradient of 2
    assert torch.equal(hmap.reshape(-1), e["raw"][3])
    # NCHW memory gives the same result
    x2 = x.detach().contiguous().requires_grad_()
    assert x2.is_contiguous()
    crit = losses.EntropyLoss(case[1], case[2])
    l3 = crit(x2)
    l3.backward()
    assert torch.equal(l3.detach(), loss.detach()) and torch.equal(crit.last_entropy, ment) and torch.equal(x2.grad * 2, x.grad)
    # without a gradient: the same scalars
    with torch.no_grad():
        l4, m4 = F.entropy_loss(x.detach(), case[1], case[2])
    assert torch.equal(l4, loss.detach()) and torch.equal(m4, ment) and not l4.requires_grad


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[3], R.CASES[15]], ids=lambda c: R.key(*c))
def test_a_world_of_two_halves_loss_and_gradient(case, monkeypatch):
    x, (loss, ment) = _fn(case)
    loss.backward()
    monkeypatch.setattr(F, "dp_world", lambda: 2)
    x2 = x.detach().clone().requires_grad_()
    loss2, ment2 = F.entropy_loss(x2, case[1], case[2])
    loss2.backward()
    assert torch.equal(loss2.detach() * 2, loss.detach()) and torch.equal(ment2 * 2, ment) and torch.equal(x2.grad * 2, x.grad)
    assert float(loss.detach()) != 0.0 and bool(x.grad.any())


def test_refusals():
    x = torch.zeros((2, 19, 4, 4), device=DEV)
    with pytest.raises(RuntimeError, match=r"\[n, c, h, w\]"):
        F.entropy_loss(x[0])
    for c in (1, 33):
        with pytest.raises(RuntimeError, match=r"\[2, 32\]"):
            F.entropy_loss(torch.zeros((2, c, 4, 4), device=DEV))
    with pytest.raises(RuntimeError, match="dtype"):
        F.entropy_loss(x.half())
    with pytest.raises(RuntimeError, match="HIP"):
        F.entropy_loss(x.cpu())
    with pytest.raises(RuntimeError, match="penalty"):
        F.entropy_loss(x, "shannon")
    for eta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="eta"):
            F.entropy_loss(x, "robust", eta)
    with pytest.raises(RuntimeError, match="HIP"):
        F.entropy_loss(x, entropy_map=torch.zeros(2, 4, 4))
    for bad in (torch.zeros((2, 4, 5), device=DEV), torch.zeros((2, 1, 4, 4), device=DEV),
                torch.zeros((2, 4, 4), dtype=torch.float64, device=DEV), torch.zeros((2, 4, 4), dtype=torch.bfloat16, device=DEV)):
        with pytest.raises(RuntimeError, match="entropy_map"):
            F.entropy_loss(x, entropy_map=bad)


def test_graph_capture_of_forward_and_backward_replays_on_refreshed_inputs():
    n, c, h, w = R.SHAPES[1]
    x = torch.zeros((n, c, h, w), dtype=torch.bfloat16, device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    hmap = torch.zeros((n, h, w), device=DEV)
    (F.entropy_loss(x, "robust", 0.5, hmap)[0] * 1.0).backward()           # eager (and the first, warming call)
    x.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a straight line on one stream: forward, finish, backward
        loss, ment = F.entropy_loss(x, "robust", 0.5, hmap)
        dx, = torch.autograd.grad(loss, x)
    for seed in (71, 72):
        xn = R.logits((n, h, w, c), seed, "bf16")
        with torch.no_grad():
            x.copy_(_nhwc(xn, "bf16"))
        graph.replay()
        torch.cuda.synchronize()
        got = (loss.detach().clone(), ment.clone(), dx.clone(), hmap.clone())
        xe, he = x.detach().clone().requires_grad_(), torch.zeros((n, h, w), device=DEV)
        le, me = F.entropy_loss(xe, "robust", 0.5, he)
        le.backward()
        assert torch.equal(got[0], le.detach()) and torch.equal(got[1], me) and torch.equal(got[2], xe.grad) and torch.equal(got[3], he)
        want = R.entropy(xn, "robust", 0.5)
        assert abs(float(got[0]) - float(want[0])) <= 1e-5 * float(want[0]) and abs(float(got[1]) - float(want[1])) <= 1e-5 * float(want[1])


# ------------------------------------------------------------------ entmin_step
SRC, TGT = (2, 64, 128), (3, 96, 160)   # the sizes and batch sizes differ on purpose


def _load(net, seed):
    sd = net.state_dict()
    net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed))
    return net.to(DEV)


def _model(kind, seed=1):
    return _load(BiSeNet(19, "resnet18") if kind == "bisenet" else get_deeplab_v2(19, pretrain=False), seed).train()


def _batches():
    return (synthetic_images(*SRC, seed=80).to(DEV), synthetic_labels(*SRC, seed=90).to(DEV), synthetic_images(*TGT, seed=81).to(DEV))


def _state(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _same(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) for k in (keys or a))


@pytest.mark.parametrize("kind,precision", [("bisenet", torch.float32), ("deeplab", torch.bfloat16)])
def test_entmin_step(kind, precision):
    xs, ys, xt = _batches()
    crit = losses.CrossEntropyLoss(ignore_index=19)
    with rtsds_amd.precision(precision):
        em = entmin.EntropyMinimiser("robust", 2.0, 0.5)
        net = _model(kind)
        before = _state(net)
        # the same head from a twin model (train-mode forward, same parameters, BatchNorm statistics of the target batch)
        (low, _), = _model(kind).forward_lowres(xt, main_only=True)
        ent_ref, h_ref = F.entropy_loss(low.detach(), "robust", 2.0)
        loss, correct, ent, h = entmin.entmin_step(net, em, crit, optim.Adam(net.parameters(), lr=1e-3), xs, ys, xt)
        torch.cuda.synchronize()
    after = _state(net)
    assert any(not torch.equal(before[k], after[k]) for k, _ in net.named_parameters())
    assert torch.equal(ent, ent_ref) and torch.equal(h, h_ref) and not ent.requires_grad and not h.requires_grad
    assert np.isfinite(float(loss)) and float(ent) > 0 and 0.0 < float(h) <= 1.0 and 0 <= int(correct) <= 2 * 64 * 128
    print(f"{kind}: loss {float(loss):.4f}, entropy loss {float(ent):.6f}, target entropy {float(h):.4f}, low head {tuple(low.shape)}")


@pytest.mark.parametrize("kind,precision", [("bisenet", torch.float32), ("deeplab", torch.bfloat16)])
def test_weight_zero_is_seg_step(kind, precision):
    xs, ys, xt = _batches()
    crit = losses.CrossEntropyLoss(ignore_index=19)

    def seg():
        net = _model(kind)
        loss, correct = train.seg_step(net, crit, optim.Adam(net.parameters(), lr=1e-3), xs, ys)
        return _state(net), loss, correct

    with rtsds_amd.precision(precision):
        (a, la, ca), (b, lb, cb) = seg(), seg()
        assert _same(a, b) and torch.equal(la, lb) and torch.equal(ca, cb)        # the premise: seg_step repeats itself
        net = _model(kind)
        params, before = [k for k, _ in net.named_parameters()], _state(net)
        em = entmin.EntropyMinimiser("entropy", 2.0, 0.0)
        loss, correct, ent, h = entmin.entmin_step(net, em, crit, optim.Adam(net.parameters(), lr=1e-3), xs, ys, xt)
        torch.cuda.synchronize()
    after = _state(net)
    assert _same(a, after, params) and torch.equal(correct, ca) and torch.equal(loss, la) and float(ent) > 0
    # the target batch passed through the main head's BatchNorms as well: their counters moved by 2 where
    # seg_step's moved by 1 (the auxiliary heads, which the target forward leaves out, by 1), and the
    # running statistics differ
    tracked = [k for k in after if k.endswith("num_batches_tracked")]
    moved = [int(after[k]) - int(before[k]) for k in tracked]
    assert tracked and all(int(a[k]) - int(before[k]) == 1 for k in tracked)
    assert set(moved) <= {1, 2} and moved.count(2) >= 1
    assert any(not torch.equal(a[k], after[k]) for k in after if k.endswith("running_mean"))


def test_entmin_step_refuses_a_model_without_lowres_heads():
    net = torch.nn.Conv2d(3, 19, 1).to(DEV)
    xs, ys, xt = _batches()
    with pytest.raises(RuntimeError, match="forward_lowres"):
        entmin.entmin_step(net, entmin.EntropyMinimiser(), losses.CrossEntropyLoss(ignore_index=19),
                           optim.Adam(net.parameters(), lr=1e-3), xs, ys, xt)


# ------------------------------------------------------------------ main --entropy_min
def _cfg(tmp_path, precision, block):
    cfg = yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))
    cfg["precision"] = precision
    cfg["data"]["cityscapes"].update(image_size="64, 128", batch_size=2)
    cfg["data"]["gta5_modified"].update(image_size="80, 160", batch_size=2)
    cfg["data"]["synthetic_batches"] = 2
    cfg["training"]["segmentation"].update(epochs=1)
    cfg["training"]["entropy_minimisation"] = block
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


@pytest.mark.parametrize("block,precision", [({"penalty": "robust", "weight": 0.005, "eta": 2.0}, "fp32"),
                                             ({"penalty": "max_squares", "weight": 0.1, "eta": 2.0}, "bf16")])
def test_main_entropy_min(tmp_path, monkeypatch, block, precision):
    monkeypatch.chdir(tmp_path)
    seen = {"logs": [], "kw": None}
    real_train = entmin.train

    class Log(Callback):
        def on_batch_end(self, batch, logs=None):
            seen["logs"].append(dict(logs))

    def logged(**kw):
        seen["kw"] = kw
        kw["callbacks"] = list(kw["callbacks"]) + [Log()]
        return real_train(**kw)
    monkeypatch.setattr(entmin, "train", logged)
    monkeypatch.setattr(rmain, "train", lambda **kw: pytest.fail("the plain loop ran under --entropy_min"))
    before = rtsds_amd.compute_dtype()
    try:
        rmain.main(["--config", _cfg(tmp_path, precision, block), "--model", "bisenet", "--dataset", "gta5", "--entropy_min"])
    finally:
        rtsds_amd.set_compute_dtype(before)
    em = seen["kw"]["minimiser"]
    assert isinstance(em, entmin.EntropyMinimiser) and (em.penalty, em.weight, em.eta) == (block["penalty"], block["weight"], block["eta"])
    assert seen["kw"]["target_loader"] is not seen["kw"]["train_loader"]
    assert len(seen["logs"]) == 2                                               # two iterations
    for logs in seen["logs"]:
        assert np.isfinite(logs["entropy_loss"]) and 0.0 <= logs["target_entropy"] <= 1.0
        assert np.isfinite(logs["train_loss"]) and 0.0 <= logs["train_accuracy"] <= 100.0
