"""Class-weighted cross-entropy, host side (no GPU): the float64 restatement the GPU tests compare
against equals torch's own chain; the criterion's weight handling; class_weights against numbers
worked out by hand; the config forms; the new entry points' argument checks (nothing launches)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF
import yaml

from rtsds_amd import _lib, losses
from rtsds_amd import main as rmain

from tests import wce_ref as R
from tests.conv_cases import _close


# ------------------------------------------------------------------ the reference's premise
@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=R.IDS)
def test_restatement_equals_torch_fp64(idx):
    d = R.data(idx)
    resize = R.CASES[idx][4]
    hr = [h.clone().requires_grad_() for h in d.heads]
    ups = [TF.interpolate(h, mode="bilinear", align_corners=False, **resize) for h in hr]
    assert tuple(ups[0].shape[2:]) == (d.H, d.W)
    loss = sum(TF.cross_entropy(u, d.target, weight=d.weight.double(), ignore_index=R.IGNORE) for u in ups)
    loss.backward(torch.tensor(1.5, dtype=torch.float64))
    total, grads, up0 = R.reference(idx)
    _close(up0, ups[0], torch.float64, "upsample", 1e-13)
    _close(total, loss, torch.float64, "loss", 1e-13)
    for i, h in enumerate(hr):
        _close(grads[i], h.grad, torch.float64, f"dhead{i}", 1e-12)


def test_restatement_unweighted_and_label_stats():
    d = R.data(2)
    z = R.upsample(d.heads[0], d.H, d.W, d.sh, d.sw)
    loss, _, wsum = R.weighted_ce(z, d.target, None)
    _close(loss, TF.cross_entropy(z, d.target, ignore_index=R.IGNORE), torch.float64, "loss", 1e-13)
    assert float(wsum) == float((d.target != R.IGNORE).sum())
    lab = np.array([[[0, 0, 1], [255, 7, -1]], [[2, 2, 2], [2, 2, 2]]])
    count, support = R.label_stats(lab, 3, 255)
    assert count.tolist() == [2, 1, 6] and support.tolist() == [3, 3, 6]


# ------------------------------------------------------------------ the criterion
def test_criterion_accepts_list_ndarray_tensor():
    for w in ([1.0, 2.0, 0.0], np.array([1.0, 2.0, 0.0]), torch.tensor([1.0, 2.0, 0.0], dtype=torch.float64),
              (1, 2, 0)):
        crit = losses.CrossEntropyLoss(weight=w, ignore_index=19)
        assert crit.weight.dtype == torch.float32 and crit.weight.tolist() == [1.0, 2.0, 0.0]
        assert "weight" in dict(crit.named_buffers())          # .to(device) moves it
    assert losses.CrossEntropyLoss(ignore_index=19).weight is None


@pytest.mark.parametrize("bad, match", [([1.0, -0.5, 2.0], r"weight\[1\]"), ([1.0, 2.0, float("nan")], r"weight\[2\]"),
                                        ([float("inf"), 1.0], r"weight\[0\]"), ([[1.0, 2.0], [3.0, 4.0]], "1-D")])
def test_criterion_rejects_bad_weights(bad, match):
    with pytest.raises(ValueError, match=match):
        losses.CrossEntropyLoss(weight=bad)


def test_criterion_rejects_wrong_length_and_other_reductions():
    crit = losses.CrossEntropyLoss(weight=[1.0] * 18, ignore_index=19)
    with pytest.raises(ValueError, match="18 class weights for 19 classes"):   # before any device work
        crit(torch.zeros(1, 19, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        losses.CrossEntropyLoss(reduction="sum")
    with pytest.raises(NotImplementedError):
        losses.CrossEntropyLoss(weight=[1.0, 1.0], reduction="sum")


def test_set_weight_validates_and_replaces():
    crit = losses.CrossEntropyLoss(ignore_index=19)
    crit.set_weight(np.array([0.5, 2.0]))
    assert crit.weight.tolist() == [0.5, 2.0] and crit.weight.dtype == torch.float32
    with pytest.raises(ValueError, match=r"weight\[0\]"):
        crit.set_weight([-1.0, 1.0])
    crit.set_weight(None)
    assert crit.weight is None


# ------------------------------------------------------------------ class_weights, by hand
def test_class_weights_inverse_log():
    # p = (0.1, 0.3, 0, 0.6): w = 1 / ln(1.02 + p); the absent class gets 1 / ln(1.02)
    w = losses.class_weights([10, 30, 0, 60], mode="inverse_log")
    want = [1 / math.log(1.12), 1 / math.log(1.32), 1 / math.log(1.02), 1 / math.log(1.62)]
    assert w.dtype == np.float64 and np.allclose(w, want, rtol=1e-15, atol=0)
    assert abs(w[2] - 50.498) < 1e-3


def test_class_weights_median_frequency():
    # two images of 100 valid pixels: class 0 in both (30 + 50), class 1 in the first only (70),
    # class 2 absent, class 3 in the second only (50)
    count, support = [80, 70, 0, 50], [200, 100, 0, 100]
    # f = (0.4, 0.7, -, 0.5): median 0.5
    w = losses.class_weights(count, support, "median_frequency")
    assert np.allclose(w, [0.5 / 0.4, 0.5 / 0.7, 0.0, 1.0], rtol=1e-15, atol=0)
    with pytest.raises(ValueError, match="support"):
        losses.class_weights(count, None, "median_frequency")
    with pytest.raises(ValueError, match="unknown mode"):
        losses.class_weights(count, support, "balanced")
    with pytest.raises(ValueError, match="no labelled pixel"):
        losses.class_weights([0, 0], [0, 0], "inverse_log")


def test_class_weights_from_the_reference_statistics():
    lab = np.full((2, 10, 10), 255)
    lab[0, :3] = 0
    lab[0, 3:] = 1
    lab[1, :5] = 0
    lab[1, 5:] = 3
    count, support = R.label_stats(lab, 4, 255)
    assert count.tolist() == [80, 70, 0, 50] and support.tolist() == [200, 100, 0, 100]


# ------------------------------------------------------------------ config
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


ADAM = {"name": "Adam", "lr": 1e-4}


def test_config_list_form_is_installed_directly():
    w = [0.5 + 0.1 * k for k in range(19)]
    _, crit = rmain.optimzer_loss_loader(_Net(), ADAM, {"name": "CrossEntropy", "ignore_index": 19, "weight": w}, 19)
    assert crit.weight_mode is None and np.allclose(crit.weight.numpy(), np.float32(w)) and crit.ignore_index == 19
    _, plain = rmain.optimzer_loss_loader(_Net(), ADAM, {"name": "CrossEntropy", "ignore_index": 19})
    assert plain.weight is None and plain.weight_mode is None


@pytest.mark.parametrize("mode", losses.WEIGHT_MODES)
def test_config_string_forms_wait_for_the_label_sweep(mode, monkeypatch, capsys):
    _, crit = rmain.optimzer_loss_loader(_Net(), ADAM, {"name": "CrossEntropy", "ignore_index": 19, "weight": mode}, 19)
    assert crit.weight is None and crit.weight_mode == mode
    count = np.arange(1, 20, dtype=np.int64) * 100
    support = np.full(19, int(count.sum()), dtype=np.int64)
    monkeypatch.setattr(losses, "class_statistics", lambda loader, c, ignore, device: (count, support))
    names = [f"class{k}" for k in range(19)]
    w = rmain.install_class_weights(crit, [], 19, names, "cpu")
    assert np.array_equal(w, losses.class_weights(count, support, mode))
    assert np.array_equal(crit.weight.numpy(), np.float32(w))
    out = capsys.readouterr().out
    assert mode in out and all(n in out for n in names)
    # a criterion without a mode is left alone
    assert rmain.install_class_weights(losses.CrossEntropyLoss(ignore_index=19), [], 19, names, "cpu") is None


def test_config_bad_string_and_bad_length_raise_at_startup():
    with pytest.raises(ValueError, match="'inverse_log'"):
        rmain.optimzer_loss_loader(_Net(), ADAM, {"name": "CrossEntropy", "ignore_index": 19, "weight": "balanced"}, 19)
    with pytest.raises(ValueError, match="18 entries for 19 classes"):
        rmain.optimzer_loss_loader(_Net(), ADAM, {"name": "CrossEntropy", "ignore_index": 19, "weight": [1.0] * 18}, 19)
    with pytest.raises(ValueError, match="list of class weights"):
        rmain.optimzer_loss_loader(_Net(), ADAM, {"name": "CrossEntropy", "ignore_index": 19, "weight": 2.0}, 19)


def test_shipped_config_carries_the_key_commented_out():
    text = open(rmain.argumnet_parser([]).config).read()
    assert '# criterion: {name: "CrossEntropy", ignore_index: 19, weight: "inverse_log"}' in text
    cfg = yaml.safe_load(text)
    assert "weight" not in cfg["model"]["bisenet"]["criterion"]


# ------------------------------------------------------------------ entry points: argument checks only
OK, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 2, 4
NZ = 0x1000   # a non-null address that is never dereferenced: every check precedes any launch


def test_weighted_entry_points_report_argument_errors_without_a_gpu():
    lib = _lib.load()
    geo = (2, 8, 16, 19, 64, 128, 0.125, 0.125)                      # n, hl, wl, c, H, W, sh, sw
    nbytes = lib.rtsds_upce_workspace(3, *geo)
    assert nbytes > 0
    heads = (ctypes.c_void_p * 3)(NZ, NZ, NZ)

    def upce(weight, c, ws_bytes, ws=NZ):
        n, hl, wl, _, H, W, sh, sw = geo
        return lib.rtsds_upce_weighted_fwd(3, heads, NZ, weight, n, hl, wl, c, H, W, sh, sw, 255, NZ, NZ, None, 1, _lib.F32,
                                           ws, ws_bytes, None)
    assert upce(None, 19, nbytes) == ERR_SHAPE
    assert upce(NZ, 0, nbytes) == ERR_SHAPE
    assert upce(NZ, 33, nbytes) == ERR_SHAPE
    assert upce(NZ, 19, nbytes - 1) == ERR_WORKSPACE
    assert upce(NZ, 19, nbytes, None) == ERR_WORKSPACE

    ce_ws = lib.rtsds_ce_workspace()

    def ce(weight, c, ws_bytes):
        return lib.rtsds_ce_weighted_fwd(NZ, 240 * c, 1, c, NZ, weight, NZ, 2, 240, c, 255, _lib.F32, NZ, ws_bytes, None)
    assert ce(None, 19, ce_ws) == ERR_SHAPE
    assert ce(NZ, 0, ce_ws) == ERR_SHAPE
    assert ce(NZ, 33, ce_ws) == ERR_SHAPE
    assert ce(NZ, 19, ce_ws - 1) == ERR_WORKSPACE

    def ce_bwd(weight, c):
        return lib.rtsds_ce_weighted_bwd(NZ, 240 * c, 1, c, NZ, weight, NZ, NZ, NZ, 2, 240, c, 255, _lib.F32, None)
    assert ce_bwd(None, 19) == ERR_SHAPE
    assert ce_bwd(NZ, 0) == ERR_SHAPE
    assert ce_bwd(NZ, 33) == ERR_SHAPE


def test_label_stats_entry_point_reports_argument_errors_without_a_gpu():
    lib = _lib.load()
    assert lib.rtsds_label_stats_workspace(3, 19) > 0
    assert lib.rtsds_label_stats_workspace(3, 0) == 0 and lib.rtsds_label_stats_workspace(3, 33) == 0
    assert lib.rtsds_label_stats_workspace(0, 19) == 0
    nbytes = lib.rtsds_label_stats_workspace(3, 19)

    def stats(label, c, ws, ws_bytes, count=NZ, support=NZ, n=3, h=37, w=53):
        return lib.rtsds_label_stats(label, n, h, w, c, 19, count, support, ws, ws_bytes, None)
    assert stats(None, 19, NZ, nbytes) == ERR_SHAPE
    assert stats(NZ, 0, NZ, nbytes) == ERR_SHAPE
    assert stats(NZ, 33, NZ, nbytes) == ERR_SHAPE
    assert stats(NZ, 19, NZ, nbytes, count=None) == ERR_SHAPE
    assert stats(NZ, 19, NZ, nbytes, support=None) == ERR_SHAPE
    assert stats(NZ, 19, NZ, nbytes, h=0) == ERR_SHAPE
    assert stats(NZ, 19, NZ, nbytes - 1) == ERR_WORKSPACE
    assert stats(NZ, 19, None, nbytes) == ERR_WORKSPACE
