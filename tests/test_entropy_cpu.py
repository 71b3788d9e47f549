"""Target entropy minimisation without a GPU: the fp64 statement of tests/entropy_ref.py against
torch's own softmax / log_softmax / autograd in fp64, the pinned tolerances
(tests/pinned/entropy_tol.json), the special rows, the config block, main's refusals, and the
argument validation of the rtsds_entropy_* entries, which comes before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

import rtsds_amd
from rtsds_amd import _lib, entmin, losses
from rtsds_amd import functional as F
from rtsds_amd import main as rmain

from tests import entropy_ref as R

PINNED = R.pinned()


# ------------------------------------------------------------------ the yardstick
def torch_penalty(x, penalty, eta):
    """The three formulas in torch on NCHW logits ``x``: (loss, mean normalised entropy)."""
    c = x.shape[1]
    h = -(torch.softmax(x, 1) * torch.log_softmax(x, 1)).sum(1) / np.log(c)
    if penalty == "entropy":
        return h.mean(), h.mean()
    if penalty == "robust":
        return ((h ** 2 + 1e-8) ** eta).mean(), h.mean()
    return -0.5 * (torch.softmax(x, 1) ** 2).sum(1).mean(), h.mean()


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_fp64_statement_equals_torch_fp64_autograd(case):
    shape, penalty, eta, _ = case
    cs = R.case(*case)
    x = torch.from_numpy(cs.x.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_()
    loss, ment = torch_penalty(x, penalty, eta)
    loss.backward()
    gmax = float(np.abs(cs.grad64).max())
    e_loss, e_ent = abs(float(loss.detach()) - cs.loss64), abs(float(ment.detach()) - cs.ent64)
    e_grad = float(np.abs(x.grad.permute(0, 2, 3, 1).numpy() - cs.grad64).max())
    print(f"{R.key(*case)}: loss {e_loss:.1e} of {cs.loss64:.4f}, entropy {e_ent:.1e} of {cs.ent64:.4f}, gradient {e_grad:.1e} of {gmax:.2e}")
    assert e_loss <= 1e-12 * abs(cs.loss64) and e_ent <= 1e-12 * cs.ent64 and e_grad <= 1e-12 * gmax
    assert 0.0 <= cs.map64.min() and cs.map64.max() <= 1.0


def test_the_cases_of_the_issue_are_all_there():
    for shape in [(2, 19, 8, 16), (1, 19, 13, 17), (2, 7, 9, 40), (1, 2, 4, 4), (1, 32, 4, 4), (1, 19, 1, 1), (1, 19, 64, 128)]:
        for dt in ("f32", "bf16"):
            assert any(c[0] == shape and c[3] == dt for c in R.CASES)
    for pen in [("entropy", 2.0), ("robust", 2.0), ("robust", 0.5), ("max_squares", 2.0)]:
        assert any(c[0] == R.REAL and c[1:3] == pen for c in R.CASES)
    assert len(set(R.IDS)) == len(R.IDS)


def test_inputs_have_standard_deviation_four_and_fit_their_dtype():
    f, b = R.case(*R.CASES[-1]), R.case(*R.CASES[-2])   # the real geometry in fp32 and in bf16
    assert 3.5 < f.x.std() < 4.5 and 3.5 < b.x.std() < 4.5
    assert np.array_equal(R.to_bf16(b.x), b.x) and not np.array_equal(R.to_bf16(f.x), f.x)


# ------------------------------------------------------------------ pinned tolerances
def test_regenerating_the_pinned_file_reproduces_it():
    assert R.record() == PINNED and sorted(PINNED) == sorted(R.IDS)


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_pinned_tolerance_is_the_restatement_error_or_one_ulp(case):
    cs, p = R.case(*case), PINNED[R.key(*case)]
    assert sorted(p) == sorted(R.QUANTITIES)
    gmax = float(np.abs(cs.grad64).max())
    for q, ref, got in (("loss", cs.loss64, float(cs.loss32)), ("entropy", cs.ent64, float(cs.ent32))):
        assert p[q] >= 0.999 * float(np.spacing(np.float32(abs(ref)))) and p[q] >= 0.999 * abs(got - ref)
        assert p[q] <= 1e-5 * abs(ref)      # nothing here is loose: a few fp32 roundings per term of the sums
    assert p["grad"] >= 0.999 * float(np.spacing(np.float32(gmax))) and p["grad"] <= 1e-5 * gmax
    assert p["map"] <= 1e-6
    print(f"{R.key(*case)}: loss {p['loss'] / abs(cs.loss64):.1e} rel, entropy {p['entropy'] / cs.ent64:.1e} rel, "
          f"gradient {p['grad'] / gmax:.1e} of max, map {p['map']:.1e}")


# ------------------------------------------------------------------ special rows
@pytest.mark.parametrize("penalty,eta", R.PENALTIES)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_special_rows(penalty, eta, dt):
    x = R.special_rows()
    loss, ment, grad, h = R.entropy(x, penalty, eta, dt)
    tol = 1e-14 if dt == np.float64 else R.MARGIN * 2.0 ** -23
    assert np.isfinite(loss) and np.isfinite(ment) and np.isfinite(grad).all() and np.isfinite(h).all()
    assert 0.0 <= h.min() and h.max() <= 1.0
    # one logit at 200: in fp32 the other exponentials underflow, entropy and gradient are exactly 0
    if dt == np.float32:
        assert h[0, 0, 0] == 0.0 and not grad[0, 0, 0].any()
    else:
        assert h[0, 0, 0] < 1e-80 and np.abs(grad[0, 0, 0]).max() < 1e-80
    # a constant row: h = 1, gradient 0 (under max_squares too: p_j = S = 1 / c)
    assert abs(float(h[0, 0, 1]) - 1.0) <= tol and np.abs(grad[0, 0, 1]).max() <= tol
    # classes at -inf: no NaN, and no gradient there
    assert not grad[0, 0, 2, [1, 4, 18]].any() and grad[0, 0, 2].any() and 0.0 < h[0, 0, 2] < 1.0
    # two equal maxima: equal gradients
    assert grad[0, 0, 3, 2] == grad[0, 0, 3, 9] and 0.0 < h[0, 0, 3] < 1.0
    t = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    want = -torch.special.xlogy(torch.softmax(t, 1), torch.softmax(t, 1)).sum(1) / np.log(19)
    assert np.abs(h.astype(np.float64) - want.numpy()[0]).max() <= (1e-12 if dt == np.float64 else 1e-6)


# ------------------------------------------------------------------ C entry points
OK, SHAPE, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
_BUF = ctypes.create_string_buffer(4096 + 16)
_PTR = (ctypes.addressof(_BUF) + 15) & ~15  # dummies: validation returns before anything is dereferenced
GEO = dict(n=2, h=8, w=16, c=19)


def _fwd(**over):
    a = dict(GEO, x=_PTR, dtype=1, penalty=0, eta=2.0, want=1, hmap=None, wsp=_PTR, ws_bytes=1 << 30)
    a.update(over)
    return _lib.load().rtsds_entropy_fwd(a["x"], a["dtype"], a["n"], a["h"], a["w"], a["c"], a["penalty"], a["eta"], a["want"],
                                         a["hmap"], a["wsp"], a["ws_bytes"], None)


def _finish(**over):
    a = dict(wsp=_PTR, ws_bytes=1 << 30, n=2, h=8, w=16, coef=1.0, loss=_PTR, ment=_PTR + 4)
    a.update(over)
    return _lib.load().rtsds_entropy_finish(a["wsp"], a["ws_bytes"], a["n"], a["h"], a["w"], a["coef"], a["loss"], a["ment"], None)


def _bwd(**over):
    a = dict(GEO, wsp=_PTR, ws_bytes=1 << 30, g=_PTR, coef=1.0, dx=_PTR, dtype=1)
    a.update(over)
    return _lib.load().rtsds_entropy_bwd(a["wsp"], a["ws_bytes"], a["g"], a["coef"], a["dx"], a["dtype"], a["n"], a["h"], a["w"],
                                         a["c"], None)


def test_abi_revision_and_argument_counts():
    assert _lib.ABI_VERSION >= 27 and _lib.load().rtsds_abi_version() == _lib.ABI_VERSION
    counts = {"rtsds_entropy_workspace": 4, "rtsds_entropy_fwd": 13, "rtsds_entropy_finish": 9, "rtsds_entropy_bwd": 11}
    for name, k in counts.items():
        assert len(_lib.SIGNATURES[name][1]) == k, name
    header = open(os.path.join(os.path.dirname(rtsds_amd.__file__), "..", "include", "rtsds_hip.h")).read()
    for name, k in counts.items():
        decl = header[header.index(f" {name}("):]
        assert decl[:decl.index(");")].count(",") + 1 == k, name


def test_workspace_query():
    ws = _lib.load().rtsds_entropy_workspace
    # two fp32 partials per tile of 128 pixels (16-B multiple) and the fp32 gradient term
    assert ws(2, 8, 16, 19) == 2 * 2 * 4 + 2 * 8 * 16 * 19 * 4
    assert ws(1, 13, 17, 19) == 16 + 13 * 17 * 19 * 4
    assert ws(1, 1, 1, 19) == 16 + 19 * 4
    assert ws(8, 64, 128, 19) == 512 * 2 * 4 + 8 * 64 * 128 * 19 * 4
    for bad in [(0, 8, 16, 19), (2, 0, 16, 19), (2, 8, -1, 19), (2, 8, 16, 1), (2, 8, 16, 33), (64, 4096, 4096, 19),
                (1, 1 << 15, 1 << 15, 2)]:
        assert ws(*bad) == 0, bad


@pytest.mark.parametrize("over", [{"n": 0}, {"h": 0}, {"w": -3}, {"c": 1}, {"c": 33}, {"n": 64, "h": 4096, "w": 4096}, {"x": None},
                                  {"penalty": 3}, {"penalty": -1}, {"eta": 0.0}, {"eta": -2.0}, {"eta": float("nan")},
                                  {"eta": float("inf")}, {"penalty": 0, "eta": 0.0}])
def test_forward_entry_rejects_bad_arguments(over):
    assert _fwd(**over) == SHAPE


def test_forward_entry_dtype_alignment_workspace():
    assert _fwd(dtype=2) == UNSUPPORTED and _fwd(dtype=-1) == UNSUPPORTED
    assert _fwd(dtype=2, c=40) == SHAPE                               # a bad shape is reported first
    assert _fwd(dtype=0, x=_PTR + 2) == UNSUPPORTED                   # an fp32 tensor off its element size
    assert _fwd(x=_PTR + 1) == UNSUPPORTED and _fwd(wsp=_PTR + 8) == UNSUPPORTED and _fwd(hmap=_PTR + 2) == UNSUPPORTED
    need = _lib.load().rtsds_entropy_workspace(*[GEO[k] for k in ("n", "h", "w", "c")])
    assert _fwd(ws_bytes=need - 1) == WORKSPACE and _fwd(wsp=None) == WORKSPACE


@pytest.mark.parametrize("over", [{"n": 0}, {"h": 0}, {"w": 0}, {"loss": None}, {"ment": None}, {"coef": float("nan")},
                                  {"coef": float("inf")}])
def test_finish_entry_rejects_bad_arguments(over):
    assert _finish(**over) == SHAPE


def test_finish_entry_alignment_workspace():
    assert _finish(wsp=_PTR + 4) == UNSUPPORTED and _finish(loss=_PTR + 2) == UNSUPPORTED
    assert _finish(wsp=None) == WORKSPACE and _finish(ws_bytes=2 * 2 * 4 - 1) == WORKSPACE


@pytest.mark.parametrize("over", [{"n": 0}, {"h": 0}, {"w": 0}, {"c": 1}, {"c": 33}, {"g": None}, {"dx": None}, {"coef": float("nan")}])
def test_backward_entry_rejects_bad_arguments(over):
    assert _bwd(**over) == SHAPE


def test_backward_entry_dtype_alignment_workspace():
    assert _bwd(dtype=2) == UNSUPPORTED and _bwd(dx=_PTR + 1) == UNSUPPORTED and _bwd(dtype=0, dx=_PTR + 2) == UNSUPPORTED
    assert _bwd(wsp=_PTR + 8) == UNSUPPORTED and _bwd(g=_PTR + 2) == UNSUPPORTED
    need = _lib.load().rtsds_entropy_workspace(2, 8, 16, 19)
    assert _bwd(ws_bytes=need - 1) == WORKSPACE and _bwd(wsp=None) == WORKSPACE


# ------------------------------------------------------------------ the Python layer
def test_python_layer_refuses_host_tensors_and_bad_settings():
    x = torch.zeros(1, 19, 4, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        F.entropy_loss(x)
    with pytest.raises(RuntimeError, match="HIP"):
        losses.EntropyLoss("robust")(x)
    with pytest.raises(ValueError, match="penalty"):
        losses.EntropyLoss("shannon")
    with pytest.raises(ValueError, match="eta"):
        losses.EntropyLoss("robust", eta=0.0)
    assert rtsds_amd.EntropyMinimiser is entmin.EntropyMinimiser
    em = entmin.EntropyMinimiser("max_squares", 2, 0)
    assert (em.penalty, em.eta, em.weight) == ("max_squares", 2.0, 0.0)
    for kw, match in [({"penalty": "minent"}, "penalty"), ({"eta": 0}, "eta"), ({"eta": float("nan")}, "eta"),
                      ({"weight": -1.0}, "weight"), ({"weight": float("inf")}, "weight")]:
        with pytest.raises(ValueError, match=match):
            entmin.EntropyMinimiser(**kw)
    with pytest.raises(RuntimeError, match="minimiser"):
        entmin.train(0, torch.nn.Identity(), [], None, None, 0.1, 1)


def test_target_batches_come_from_one_iterator_restarted_when_it_runs_out():
    class Loader:
        def __init__(self):
            self.started = 0

        def __iter__(self):
            self.started += 1
            return iter([(torch.full((1,), float(i)), "label") for i in range(3)])

    em, loader = entmin.EntropyMinimiser(), Loader()
    seen = [float(em.next_target(loader)) for _ in range(7)]
    assert seen == [0.0, 1.0, 2.0, 0.0, 1.0, 2.0, 0.0] and loader.started == 3 and em.restarts == 2
    with pytest.raises(RuntimeError, match="empty"):
        em.next_target([])


# ------------------------------------------------------------------ config and main
def _config(block):
    return rmain.namedtuple("Config", ["training"])({"entropy_minimisation": block} if block is not None else {})


GOOD = {"penalty": "robust", "weight": 0.005, "eta": 2.0}


def test_config_block_validation():
    assert rmain.entropy_minimisation_config(_config(GOOD)) == GOOD
    for pen in ("entropy", "robust", "max_squares"):
        assert rmain.entropy_minimisation_config(_config(dict(GOOD, penalty=pen, weight=0, eta=1)))["penalty"] == pen
    with pytest.raises(RuntimeError, match="training.entropy_minimisation"):
        rmain.entropy_minimisation_config(_config(None))
    for k in GOOD:
        with pytest.raises(RuntimeError, match=f"lacks {k}"):
            rmain.entropy_minimisation_config(_config({q: v for q, v in GOOD.items() if q != k}))
    for over in [{"penalty": "shannon"}, {"penalty": None}, {"penalty": 1}, {"weight": -0.1}, {"weight": float("inf")},
                 {"weight": float("nan")}, {"weight": True}, {"weight": None}, {"weight": "small"}, {"eta": 0}, {"eta": -1.0},
                 {"eta": float("nan")}, {"eta": True}, {"eta": "two"}]:
        with pytest.raises(RuntimeError, match=next(iter(over))):
            rmain.entropy_minimisation_config(_config(dict(GOOD, **over)))
    assert set(rmain.ENTROPY_PENALTIES) == set(F.ENTROPY_PENALTIES)


def test_shipped_config_carries_the_commented_block():
    text = open(os.path.join(os.path.dirname(rmain.__file__), "config.yaml")).read()
    assert "entropy_minimisation" not in yaml.safe_load(text)["training"]
    lines = text.split("\n")
    at = lines.index("  # entropy_minimisation:")
    block = yaml.safe_load("\n".join(ln.replace("  # ", "", 1) for ln in lines[at:at + 4]))["entropy_minimisation"]
    assert sorted(block) == sorted(rmain.ENTROPY_MINIMISATION_KEYS) and rmain.entropy_minimisation_config(_config(block)) == block
    assert block == {"penalty": "robust", "weight": 0.005, "eta": 2.0}           # FDA's setting
    for setting in ("weight 0.001", "weight 0.1", "weight 0.005"):                # ADVENT's, Maximum Squares', FDA's
        assert setting in text


def test_main_refuses_before_any_model_is_built(tmp_path, monkeypatch):
    assert rmain.argumnet_parser(["--entropy_min"]).entropy_min and not rmain.argumnet_parser([]).entropy_min
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(rmain.__file__), "config.yaml")))
    cfg["training"]["entropy_minimisation"] = dict(GOOD)
    cfg["training"]["distillation"] = {"teacher_model": "bisenet", "teacher_weights": "none.pth", "temperature": 1.0, "weight": 1.0}
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    monkeypatch.setattr(rmain, "model_loader", lambda *a, **k: pytest.fail("a model was built"))
    monkeypatch.setattr(rmain, "datasets_loader", lambda *a, **k: pytest.fail("the loaders were built"))
    before = rtsds_amd.compute_dtype()
    try:
        with pytest.raises(RuntimeError, match="segmentation branch only"):
            rmain.main(["--config", str(p), "--dataset", "gta5", "--entropy_min", "--domain_adaptation"])
        with pytest.raises(RuntimeError, match="--distill"):
            rmain.main(["--config", str(p), "--dataset", "gta5", "--entropy_min", "--distill"])
        with pytest.raises(RuntimeError, match="--dataset gta5"):
            rmain.main(["--config", str(p), "--entropy_min"])
        del cfg["training"]["entropy_minimisation"]
        p.write_text(yaml.safe_dump(cfg))
        with pytest.raises(RuntimeError, match="training.entropy_minimisation"):
            rmain.main(["--config", str(p), "--dataset", "gta5", "--entropy_min"])
    finally:
        rtsds_amd.set_compute_dtype(before)
