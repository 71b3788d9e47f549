"""AdvEnt at step level: train.da_step(..., d_input=...), adversarial_train and main --domain_adaptation with the
config key training.domain_adaptation.discriminator_input.  The op itself is tests/test_selfinfo_gpu.py's.

BiSeNet in fp32 and DeepLab in bf16 on recipe weights, source (2, 64, 128) and target (3, 96, 160): the sizes and batch
sizes differ on purpose (the two resizes have their own geometry)."""
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from oracle.weights import recipe_state_dict, synthetic_images, synthetic_labels  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import losses, optim, train  # noqa: E402
from rtsds_amd import main as rmain  # noqa: E402
from rtsds_amd.callbacks import Callback  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402
from rtsds_amd.models.deeplabv2.deeplabv2 import get_deeplab_v2  # noqa: E402
from rtsds_amd.models.domain_shift.adversarial.model import TinyDomainDiscriminator  # noqa: E402

DEV = torch.device("cuda", 0)
SRC, TGT = (2, 64, 128), (3, 96, 160)
KINDS = [("bisenet", torch.float32), ("deeplab", torch.bfloat16)]
LAMBDA, ITERATIONS = 0.1, 2


def _load(net, seed):
    sd = net.state_dict()
    net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed))
    return net.to(DEV).train()


def _generator(kind):
    return _load(BiSeNet(19, "resnet18") if kind == "bisenet" else get_deeplab_v2(19, pretrain=False), 1)


def _discriminator():
    return _load(TinyDomainDiscriminator(19), 2)


def _batches():
    return (synthetic_images(*SRC, seed=80).to(DEV), synthetic_labels(*SRC, seed=90).to(DEV), synthetic_images(*TGT, seed=81).to(DEV))


def _state(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _same(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) for k in (keys or a))


def _step(kind, lambda_=LAMBDA, disc=None, **kw):
    """One da_step on fresh models: (generator state, discriminator state, the five returned tensors, the models)."""
    xs, ys, xt = _batches()
    g, d = _generator(kind), disc if disc is not None else _discriminator()
    out = train.da_step(g, d, optim.Adam(g.parameters(), lr=1e-3), optim.Adam(d.parameters(), lr=1e-3, weight_decay=1e-4),
                        losses.CrossEntropyLoss(ignore_index=19), losses.BCEWithLogitsLoss(), xs, ys, xt, lambda_, ITERATIONS, **kw)
    torch.cuda.synchronize()
    return _state(g), _state(d), out, (g, d)


@pytest.mark.parametrize("kind,precision", KINDS)
def test_the_default_input_is_softmax_bit_for_bit(kind, precision):
    with rtsds_amd.precision(precision):
        g0, d0, out0, _ = _step(kind)
        g1, d1, out1, _ = _step(kind, d_input="softmax")
    assert _same(g0, g1) and _same(d0, d1) and len(out0) == len(out1) == 5
    assert all(torch.equal(a, b) for a, b in zip(out0, out1))


@pytest.mark.parametrize("kind,precision", KINDS)
def test_self_information_step(kind, precision):
    xs, ys, xt = _batches()
    bce = losses.BCEWithLogitsLoss()
    with rtsds_amd.precision(precision):
        before_g, before_d = _state(_generator(kind)), _state(_discriminator())
        g1, d1, out, (g, d) = _step(kind, d_input="self_information")
        # the same adversarial loss from twin models: train-mode forward of the target batch, the new op, the frozen D
        (low, geo), = _generator(kind).forward_lowres(xt, main_only=True)
        with torch.no_grad():
            pred = _discriminator()(F.upsample_self_information(low.detach(), geo))
            l_adv = LAMBDA * bce(pred, torch.ones(pred.size(), device=DEV)) / ITERATIONS
        torch.cuda.synchronize()
    l_seg, got_adv, l_dsrc, l_dtgt, correct = out
    print(f"{kind}: l_seg {float(l_seg):.5f} l_adv {float(got_adv):.6f} (twin {float(l_adv):.6f}) l_dsrc {float(l_dsrc):.5f} l_dtgt {float(l_dtgt):.5f}")
    assert torch.equal(got_adv, l_adv)
    assert all(np.isfinite(float(v)) for v in (l_seg, got_adv, l_dsrc, l_dtgt)) and 0 <= int(correct) <= SRC[0] * SRC[1] * SRC[2]
    assert any(not torch.equal(before_g[k], g1[k]) for k, _ in g.named_parameters())
    assert any(not torch.equal(before_d[k], d1[k]) for k, _ in d.named_parameters())
    # and it is another game than the softmax one
    with rtsds_amd.precision(precision):
        _, d0, out0, _ = _step(kind)
    assert not torch.equal(out0[1], got_adv) and not _same(d0, d1)


@pytest.mark.parametrize("kind,precision", KINDS)
def test_with_lambda_zero_the_generator_does_not_see_the_input(kind, precision):
    with rtsds_amd.precision(precision):
        g0, d0, out0, (g, d) = _step(kind, lambda_=0.0)
        g1, d1, out1, _ = _step(kind, lambda_=0.0, d_input="self_information")
    params = [k for k, _ in g.named_parameters()]
    assert _same(g0, g1, params) and torch.equal(out0[0], out1[0]) and float(out1[1]) == 0.0     # the adversarial gradient is an exact zero
    assert any(not torch.equal(d0[k], d1[k]) for k, _ in d.named_parameters())                    # D trained on other maps


def test_a_discriminator_without_padded_input_is_refused_with_self_information():
    disc = _discriminator()
    disc.accepts_padded_probs = False
    with rtsds_amd.precision(torch.float32):
        with pytest.raises(RuntimeError, match="accepts_padded_probs"):
            _step("bisenet", disc=disc, d_input="self_information")
        _, _, out, _ = _step("bisenet", disc=disc, d_input="softmax")           # the unfused path still serves softmax
    assert all(np.isfinite(float(v)) for v in out[:4])
    with pytest.raises(ValueError, match="d_input"):
        _step("bisenet", d_input="entropy")


# ------------------------------------------------------------------ main --domain_adaptation
def _cfg(tmp_path, value):
    cfg = yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))
    cfg["precision"] = "bf16"
    cfg["data"]["cityscapes"].update(image_size="64, 128", batch_size=2)
    cfg["data"]["gta5_modified"].update(image_size="64, 128", batch_size=2)
    cfg["data"]["synthetic_batches"] = 2
    cfg["training"]["domain_adaptation"].update(iterations=2, epochs=1, do_validation=0)
    if value is not None:
        cfg["training"]["domain_adaptation"]["discriminator_input"] = value
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


@pytest.mark.parametrize("value,want", [("self_information", "self_information"), (None, "softmax")])
def test_main_passes_the_config_key_on(tmp_path, monkeypatch, value, want):
    monkeypatch.chdir(tmp_path)
    seen = {"logs": [], "kw": None}
    real = rmain.adversarial_train

    class Log(Callback):
        def on_batch_end(self, batch, logs=None):
            seen["logs"].append(dict(logs))

    def logged(**kw):
        seen["kw"] = kw
        kw["callbacks"] = list(kw["callbacks"]) + [Log()]
        return real(**kw)
    monkeypatch.setattr(rmain, "adversarial_train", logged)
    before = rtsds_amd.compute_dtype()
    try:
        rmain.main(["--config", _cfg(tmp_path, value), "--domain_adaptation"])
    finally:
        rtsds_amd.set_compute_dtype(before)
    assert seen["kw"]["d_input"] == want
    assert len(seen["logs"]) == 2                                               # two iterations
    for logs in seen["logs"]:
        assert all(np.isfinite(logs[k]) for k in ("loss_gen_source", "loss_adversarial", "loss_disc_source", "loss_disc_target"))


def test_main_refuses_an_unknown_value_at_start_up(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(rmain, "datasets_loader", lambda *a, **k: pytest.fail("the loaders were built before the check"))
    before = rtsds_amd.compute_dtype()
    try:
        with pytest.raises(RuntimeError, match="discriminator_input"):
            rmain.main(["--config", _cfg(tmp_path, "entropy"), "--domain_adaptation"])
    finally:
        rtsds_amd.set_compute_dtype(before)
