"""Knowledge distillation without a GPU: the fp64 statement of tests/distill_ref.py against torch's
own interpolate / kl_div / autograd in fp64, the pinned tolerances and the premises of the GPU tests
(tests/pinned/distill_tol.json, no near-tie in a resampled row), the xlogy rule, the config block,
and the argument validation of the rtsds_distill_* entries, which comes before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF
import yaml

import rtsds_amd
from rtsds_amd import _lib, distill, losses
from rtsds_amd import functional as F
from rtsds_amd import main as rmain

from tests import distill_ref as R

PINNED = R.pinned()


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_fp64_statement_equals_torch_fp64_autograd(case):
    (n, c, hs, ws, ht, wt), temp, _, _ = case
    cs = R.case(*case)
    s = torch.from_numpy(cs.s.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_()
    t = torch.from_numpy(cs.t.astype(np.float64)).permute(0, 3, 1, 2)
    u = TF.interpolate(t, size=(hs, ws), mode="bilinear", align_corners=False)
    loss = TF.kl_div(TF.log_softmax(s / temp, 1), TF.softmax(u / temp, 1), reduction="sum") * temp * temp / (n * hs * ws)
    loss.backward()
    e_loss = abs(float(loss.detach()) - cs.loss64)
    e_grad = float(np.abs(s.grad.permute(0, 2, 3, 1).numpy() - cs.grad64).max())
    print(f"{R.key(*case)}: loss {e_loss:.1e} of {cs.loss64:.4f}, gradient {e_grad:.1e} of {np.abs(cs.grad64).max():.2e}")
    assert e_loss <= 1e-13 * cs.loss64 and e_grad <= 1e-13 * float(np.abs(cs.grad64).max())
    assert np.array_equal(np.argmax(u.permute(0, 2, 3, 1).numpy(), -1), np.argmax(cs.u64, -1))


def test_the_shapes_of_the_issue_are_all_there():
    for shape in [(2, 19, 8, 16, 9, 17), (1, 19, 13, 17, 13, 17), (2, 7, 9, 40, 5, 21), (1, 32, 4, 4, 7, 3), (1, 2, 4, 4, 2, 2),
                  (1, 19, 3, 300, 5, 77), (1, 19, 2, 260, 2, 4200), (1, 19, 64, 128, 65, 129)]:
        for dt in ("f32", "bf16"):
            assert any(c[0] == shape and c[2] == dt and c[3] == dt for c in R.CASES)
    assert {c[1] for c in R.CASES} == {0.5, 1.0, 4.0}
    assert any(c[2] == "f32" and c[3] == "bf16" for c in R.CASES)
    assert len(set(R.IDS)) == len(R.IDS)


# ------------------------------------------------------------------ pinned tolerances and premises
def test_regenerating_the_pinned_file_reproduces_it():
    fresh = R.record()
    assert sorted(fresh) == sorted(PINNED) == sorted(R.IDS)
    for k in R.IDS:
        for q in ("loss", "grad"):
            assert fresh[k][q] == pytest.approx(PINNED[k][q], rel=1e-3), (k, q)


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_pinned_tolerance_is_the_restatement_error_or_one_ulp(case):
    cs = R.case(*case)
    p = PINNED[R.key(*case)]
    gmax = float(np.abs(cs.grad64).max())
    assert p["loss"] >= 0.999 * float(np.spacing(np.float32(cs.loss64))) and p["grad"] >= 0.999 * float(np.spacing(np.float32(gmax)))
    assert p["loss"] >= 0.999 * abs(float(cs.loss32) - cs.loss64)
    # nothing here is loose: the restatement stays within a few fp32 roundings per term of the sums
    assert p["loss"] <= 1e-5 * cs.loss64 or case[0][5] >= 2000
    print(f"{R.key(*case)}: loss {p['loss'] / cs.loss64:.1e} rel, gradient {p['grad'] / gmax:.1e} of max")


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_no_resampled_row_has_a_near_tie(case):
    """`agree` is compared exactly: the two largest values of every resampled teacher row lie at
    least 1e-4 and four times the fp32 resample's own error apart (identity taps are exact, so
    their ties, if any, fall the same way), and the fp32 restatement counts what fp64 counts."""
    (n, c, hs, ws, ht, wt), _, _, _ = case
    cs = R.case(*case)
    gap, uerr = R.tie_margin(cs)
    print(f"{R.key(*case)}: smallest top gap {gap:.2e}, max |u32 - u64| {uerr:.1e}, agree {cs.agree} of {n * hs * ws}")
    if (hs, ws) == (ht, wt):
        assert uerr == 0.0
    else:
        assert gap >= max(1e-4, 4.0 * uerr)
    assert cs.agree32 == cs.agree


def test_inputs_have_standard_deviation_four_and_fit_their_dtype():
    cs = R.case(*R.CASES[-1])  # fp32 student, bf16 teacher
    assert 3.5 < cs.s.std() < 4.5 and 3.5 < cs.t.std() < 4.5
    assert np.array_equal(R.to_bf16(cs.t), cs.t) and not np.array_equal(R.to_bf16(cs.s), cs.s)
    x = torch.randn(1000) * 4
    assert np.array_equal(R.to_bf16(x.numpy()), x.bfloat16().float().numpy())


# ------------------------------------------------------------------ the xlogy rule
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_a_teacher_logit_of_minus_infinity_and_a_gap_of_1e4_give_a_finite_loss(dt):
    rng = np.random.default_rng(5)
    s = rng.standard_normal((1, 3, 4, 5)).astype(np.float32)
    t = rng.standard_normal((1, 3, 4, 5)).astype(np.float32)   # equal sizes: the second taps have weight zero and are left out
    t[0, 1, 2, 0] = -np.inf
    t[0, 0, 0, 3] = 1e4
    s[0, 2, 1, 4] = -1e4
    loss, grad, _, _ = R.distill(s, t, 1.0, dt)
    assert np.isfinite(loss) and loss > 0 and np.isfinite(grad).all()
    ts = torch.from_numpy(s.astype(np.float64)).permute(0, 3, 1, 2)
    tt = torch.from_numpy(t.astype(np.float64)).permute(0, 3, 1, 2)
    want = float(TF.kl_div(TF.log_softmax(ts, 1), TF.softmax(tt, 1), reduction="sum") / 12)
    assert abs(float(loss) - want) <= (1e-12 if dt == np.float64 else 1e-5) * want


# ------------------------------------------------------------------ C entry points
OK, SHAPE, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
_BUF = ctypes.create_string_buffer(4096 + 16)
_PTR = (ctypes.addressof(_BUF) + 15) & ~15  # dummies: validation returns before anything is dereferenced
GEO = dict(n=2, hs=8, ws=16, c=19, ht=9, wt=17)


def _fwd(**over):
    a = dict(GEO, s=_PTR, sd=0, t=_PTR, td=1, sh=9 / 8, sw=17 / 16, it=1.0, want=1, agree=None, wsp=_PTR, ws_bytes=1 << 30)
    a.update(over)
    return _lib.load().rtsds_distill_fwd(a["s"], a["sd"], a["t"], a["td"], a["n"], a["hs"], a["ws"], a["c"], a["ht"], a["wt"],
                                         a["sh"], a["sw"], a["it"], a["want"], a["agree"], a["wsp"], a["ws_bytes"], None)


def _finish(**over):
    a = dict(wsp=_PTR, ws_bytes=1 << 30, n=2, hs=8, ws=16, coef=1.0, loss=_PTR)
    a.update(over)
    return _lib.load().rtsds_distill_finish(a["wsp"], a["ws_bytes"], a["n"], a["hs"], a["ws"], a["coef"], a["loss"], None)


def _bwd(**over):
    a = dict(wsp=_PTR, ws_bytes=1 << 30, g=_PTR, coef=1.0, dx=_PTR, dtype=1, n=2, hs=8, ws=16, c=19)
    a.update(over)
    return _lib.load().rtsds_distill_bwd(a["wsp"], a["ws_bytes"], a["g"], a["coef"], a["dx"], a["dtype"], a["n"], a["hs"],
                                         a["ws"], a["c"], None)


def test_abi_revision():
    assert _lib.ABI_VERSION >= 25 and _lib.load().rtsds_abi_version() == _lib.ABI_VERSION


def test_workspace_query():
    ws = _lib.load().rtsds_distill_workspace
    # one fp32 partial per tile (16-B multiple) and the fp32 residual
    assert ws(2, 8, 16, 19, 9, 17) == 16 * 4 + 2 * 8 * 16 * 19 * 4
    assert ws(1, 3, 300, 19, 5, 77) == 48 + 3 * 300 * 19 * 4
    assert ws(8, 64, 128, 19, 65, 129) == 512 * 4 + 8 * 64 * 128 * 19 * 4
    for bad in [(0, 8, 16, 19, 9, 17), (2, 0, 16, 19, 9, 17), (2, 8, -1, 19, 9, 17), (2, 8, 16, 1, 9, 17), (2, 8, 16, 33, 9, 17),
                (2, 8, 16, 19, 0, 17), (2, 8, 16, 19, 9, 0), (64, 4096, 4096, 19, 9, 17), (2, 8, 16, 19, 40000, 40000)]:
        assert ws(*bad) == 0, bad


BAD = [{"n": 0}, {"hs": 0}, {"ws": -3}, {"ht": 0}, {"wt": 0}, {"c": 1}, {"c": 33}, {"n": 64, "hs": 4096, "ws": 4096}]


@pytest.mark.parametrize("over", BAD + [{"s": None}, {"t": None}, {"sh": 0.0}, {"sw": -1.0}, {"sh": float("nan")}, {"sw": float("inf")},
                                        {"it": 0.0}, {"it": -2.0}, {"it": float("nan")}, {"it": float("inf")}])
def test_forward_entry_rejects_bad_arguments(over):
    assert _fwd(**over) == SHAPE


def test_forward_entry_dtype_alignment_workspace():
    assert _fwd(sd=2) == UNSUPPORTED and _fwd(td=-1) == UNSUPPORTED
    assert _fwd(sd=2, c=40) == SHAPE                                  # a bad shape is reported first
    assert _fwd(s=_PTR + 2) == UNSUPPORTED                            # an fp32 tensor off its element size
    assert _fwd(t=_PTR + 1) == UNSUPPORTED and _fwd(wsp=_PTR + 8) == UNSUPPORTED and _fwd(agree=_PTR + 4) == UNSUPPORTED
    need = _lib.load().rtsds_distill_workspace(*[GEO[k] for k in ("n", "hs", "ws", "c", "ht", "wt")])
    assert _fwd(ws_bytes=need - 1) == WORKSPACE and _fwd(wsp=None) == WORKSPACE


@pytest.mark.parametrize("over", [{"n": 0}, {"hs": 0}, {"ws": 0}, {"loss": None}, {"coef": float("nan")}, {"coef": float("inf")}])
def test_finish_entry_rejects_bad_arguments(over):
    assert _finish(**over) == SHAPE


def test_finish_entry_alignment_workspace():
    assert _finish(wsp=_PTR + 4) == UNSUPPORTED
    assert _finish(wsp=None) == WORKSPACE and _finish(ws_bytes=16 * 4 - 1) == WORKSPACE


@pytest.mark.parametrize("over", [{"n": 0}, {"hs": 0}, {"ws": 0}, {"c": 1}, {"c": 33}, {"g": None}, {"dx": None}, {"coef": float("nan")}])
def test_backward_entry_rejects_bad_arguments(over):
    assert _bwd(**over) == SHAPE


def test_backward_entry_dtype_alignment_workspace():
    assert _bwd(dtype=2) == UNSUPPORTED and _bwd(dx=_PTR + 1) == UNSUPPORTED and _bwd(dtype=0, dx=_PTR + 2) == UNSUPPORTED
    assert _bwd(wsp=_PTR + 8) == UNSUPPORTED and _bwd(g=_PTR + 2) == UNSUPPORTED
    need = _lib.load().rtsds_distill_workspace(2, 8, 16, 19, 1, 1)
    assert _bwd(ws_bytes=need - 1) == WORKSPACE and _bwd(wsp=None) == WORKSPACE


# ------------------------------------------------------------------ the Python layer
def test_python_layer_refuses_host_tensors():
    s, t = torch.zeros(1, 19, 4, 4), torch.zeros(1, 19, 5, 5)
    with pytest.raises(RuntimeError, match="HIP"):
        F.distill_kl(s, t)
    with pytest.raises(RuntimeError, match="HIP"):
        losses.DistillationLoss(2.0)(s, t)
    with pytest.raises(ValueError, match="temperature"):
        losses.DistillationLoss(0.0)


class _Lowres(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.bn = torch.nn.BatchNorm2d(3)

    def forward_lowres(self, x, main_only=False):
        return [(self.bn(x), None)]


def test_distiller_freezes_its_teacher_and_keeps_it_in_eval():
    teacher = _Lowres().train()
    d = distill.Distiller(teacher, temperature=2.0, weight=0.5)
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters())
    assert (d.temperature, d.weight) == (2.0, 0.5)
    teacher.train()
    before = {k: v.clone() for k, v in teacher.state_dict().items()}
    head = d.teacher_head(torch.randn(2, 3, 4, 4))
    assert not teacher.training and not head.requires_grad
    assert all(torch.equal(v, before[k]) for k, v in teacher.state_dict().items())   # the running statistics did not move
    with pytest.raises(RuntimeError, match="forward_lowres"):
        distill.Distiller(torch.nn.Conv2d(3, 3, 1))
    with pytest.raises(ValueError, match="temperature"):
        distill.Distiller(_Lowres(), temperature=0.0)
    with pytest.raises(ValueError, match="weight"):
        distill.Distiller(_Lowres(), weight=-1.0)
    with pytest.raises(RuntimeError, match="distiller"):
        distill.train(0, _Lowres(), [], None, None, 0.1, 1)


# ------------------------------------------------------------------ config
def _config(block):
    return rmain.namedtuple("Config", ["training"])({"distillation": block} if block is not None else {})


GOOD = {"teacher_model": "deeplab", "teacher_weights": "teacher.pth", "temperature": 2.0, "weight": 0.5}


def test_config_block_validation():
    assert rmain.distillation_config(_config(GOOD)) == GOOD
    assert rmain.distillation_config(_config(dict(GOOD, teacher_model="bisenet", weight=0, temperature=1)))["weight"] == 0
    with pytest.raises(RuntimeError, match="training.distillation"):
        rmain.distillation_config(_config(None))
    for k in GOOD:
        with pytest.raises(RuntimeError, match=f"lacks {k}"):
            rmain.distillation_config(_config({q: v for q, v in GOOD.items() if q != k}))
    for over in [{"teacher_model": "resnet"}, {"temperature": 0}, {"temperature": -1.0}, {"temperature": "hot"},
                 {"temperature": float("nan")}, {"temperature": True}, {"weight": -0.1}, {"weight": float("inf")},
                 {"weight": None}, {"teacher_weights": ""}, {"teacher_weights": 3}]:
        with pytest.raises(RuntimeError, match=next(iter(over))):
            rmain.distillation_config(_config(dict(GOOD, **over)))


def test_build_distiller_needs_the_weights_file(tmp_path):
    with pytest.raises(RuntimeError, match="does not exist"):
        rmain.build_distiller(None, dict(GOOD, teacher_weights=str(tmp_path / "none.pth")))


def test_distill_flag_is_for_the_segmentation_branch(tmp_path):
    assert rmain.argumnet_parser(["--distill"]).distill and not rmain.argumnet_parser([]).distill
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(rmain.__file__), "config.yaml")))
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    before = rtsds_amd.compute_dtype()
    try:
        with pytest.raises(RuntimeError, match="segmentation branch only"):
            rmain.main(["--config", str(p), "--distill", "--domain_adaptation"])
        with pytest.raises(RuntimeError, match="training.distillation"):
            rmain.main(["--config", str(p), "--distill"])
    finally:
        rtsds_amd.set_compute_dtype(before)


def test_shipped_config_carries_the_commented_block():
    text = open(os.path.join(os.path.dirname(rmain.__file__), "config.yaml")).read()
    assert "distillation" not in yaml.safe_load(text)["training"]
    lines = text.split("\n")
    at = lines.index("  # distillation:")
    block = yaml.safe_load("\n".join(ln.replace("  # ", "", 1) for ln in lines[at:at + 5]))["distillation"]
    assert sorted(block) == sorted(rmain.DISTILLATION_KEYS) and rmain.distillation_config(_config(block)) == block
