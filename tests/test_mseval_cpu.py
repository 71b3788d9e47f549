"""Multi-scale / flip evaluation, host side (no GPU): the scaled sizes, the C entry point's
argument checks (which return before any launch) and the config / CLI plumbing."""
import ctypes

import pytest
import yaml

from rtsds_amd import _lib
from rtsds_amd import main as rmain
from rtsds_amd import validation

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def test_scaled_size_standard_scales():
    got = [validation.scaled_size((512, 1024), s) for s in SCALES]
    assert got == [(256, 512), (384, 768), (512, 1024), (640, 1280), (768, 1536), (896, 1792)]
    # 64 x 128: each side goes to the nearest multiple of 32, Python round() (ties to even:
    # 48/32 = 1.5 -> 2, 80/32 = 2.5 -> 2, 112/32 = 3.5 -> 4)
    got = [validation.scaled_size((64, 128), s) for s in SCALES]
    assert got == [(32, 64), (64, 96), (64, 128), (64, 160), (96, 192), (128, 224)]
    assert validation.scaled_size((64, 128), 0.1) == (32, 32)  # the align floor
    assert validation.scaled_size((64, 128), 0.25) == (32, 32)
    assert validation.scaled_size((64, 128), 0.5, align=8) == (32, 64)
    assert validation.scaled_size((100, 200), 1.0, align=8) == (96, 200)  # 12.5 -> 12


def _acc_call(x=1 << 20, acc=1 << 21, pred=None, n=1, hi=4, wi=4, c=19, ho=8, wo=8, dtype=_lib.F32):
    fn = _lib.load().rtsds_upsoftmax_acc
    return fn(x, acc, pred, n, hi, wi, c, ho, wo, 0.5, 0.5, 0, 0, dtype, None)


def test_upsoftmax_acc_rejects_bad_arguments_before_launch():
    """No device is needed: every one of these returns from the host-side checks (the pointers
    are never dereferenced)."""
    SHAPE, UNSUPPORTED = 1, 2
    assert _acc_call(c=33) == SHAPE
    assert _acc_call(n=0) == SHAPE
    assert _acc_call(ho=0) == SHAPE
    assert _acc_call(wi=-1) == SHAPE
    assert _acc_call(dtype=7) == UNSUPPORTED
    assert _acc_call(acc=None) == UNSUPPORTED
    assert _acc_call(x=None) == UNSUPPORTED


def test_upsoftmax_acc_is_bound():
    res, args = _lib.SIGNATURES["rtsds_upsoftmax_acc"]
    assert res is ctypes.c_int and len(args) == 15
    assert _lib.ABI_VERSION >= 11


def _run_main(tmp_path, monkeypatch, extra):
    cfg = yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))
    assert "eval_scales" not in cfg["training"]["segmentation"]  # commented out by default
    assert "eval_flip" not in cfg["training"]["segmentation"]
    cfg["training"]["segmentation"].update(epochs=1, **extra)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    seen = {}
    monkeypatch.setattr(rmain, "datasets_loader", lambda config, aug: ([0], [0], [0]))
    monkeypatch.setattr(rmain, "model_loader", lambda config, da, name: (object(), None, None,
                                                                         {"init_lr": 1e-4, "power": 0.9}))
    monkeypatch.setattr(rmain, "train", lambda **kw: None)
    monkeypatch.setattr(rmain, "val", lambda **kw: seen.update(kw))
    rmain.main(["--config", str(p)])
    return seen


def test_main_without_eval_keys_passes_single_scale(tmp_path, monkeypatch):
    seen = _run_main(tmp_path, monkeypatch, {})
    assert seen["scales"] is None and seen["flip"] is False


def test_main_threads_eval_keys(tmp_path, monkeypatch):
    seen = _run_main(tmp_path, monkeypatch, {"eval_scales": [0.5, 1.0], "eval_flip": True})
    assert list(seen["scales"]) == [0.5, 1.0] and seen["flip"] is True


def test_predict_multiscale_refuses_model_without_lowres_head():
    import torch
    with pytest.raises(RuntimeError, match="forward_lowres"):
        validation.predict_multiscale(torch.nn.Identity(), torch.zeros(1, 3, 32, 32), (32, 32))
