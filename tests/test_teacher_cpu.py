"""Online mean-teacher self-training, CPU side: the numpy restatements on hand-computed cases,
the decay schedule, the mode: online config plumbing and the argument checks (no HIP device)."""
from collections import namedtuple

import numpy as np
import pytest
import torch
import yaml

from rtsds_amd import _lib, ema, selftrain
from rtsds_amd import functional as F
from rtsds_amd import main as rmain
from tests import teacher_ref as R

f32 = np.float32


# ----------------------------------------------------------------------------- restatements
def test_ema_ref_hand_cases():
    t = np.array([1.0, -2.0, 0.5, 3.0e8], f32)
    s = np.array([3.0, 2.0, 0.5, -1.0], f32)
    out, _ = R.ema_ref(t, s, 0.0)
    assert np.array_equal(out, t)  # w = 0 leaves t as it was
    out, _ = R.ema_ref(t[:3], s[:3], 1.0)
    assert np.array_equal(out, s[:3])  # w = 1 copies s where s - t is exact
    out, _ = R.ema_ref(t[:3], s[:3], 0.5)
    assert np.array_equal(out, np.array([2.0, 0.0, 0.5], f32))
    # three roundings, not a fused form: w * (s - t) is rounded before the add
    w = f32(0.01)
    tt, ss = f32(1.0), f32(1.0) + f32(2.0) ** -23 * 3
    d = f32(ss - tt)
    assert R.ema_ref([tt], [ss], w)[0][0] == f32(tt + f32(w * d))


def test_bf16_bits_round_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0], f32)
    # 1.0 -> 0x3F80; the exact tie above it goes to the even 0x3F80; the tie above 0x3F81 goes up to
    # the even 0x3F82; just above a tie rounds up; -3.0 = 0xC040
    assert R.bf16_bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0xC040]
    big = np.random.default_rng(0).standard_normal(4096).astype(f32) * f32(37.0)
    ref = torch.from_numpy(big).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(big), ref)


def test_pseudo_ref_hand_cases():
    nan = f32("nan")
    p = np.array([[0.25, 0.5, 0.25, 0.0],     # plain: class 1, conf 0.5 -> bin 8 of 16
                  [0.4, 0.1, 0.4, 0.1],       # a tie takes the first class
                  [0.1, nan, 0.9, nan],       # a NaN beats every number, the first NaN wins: bin 0
                  [0.0, 0.0, 1.0, 0.0],       # conf = 1.0 -> bin bins - 1
                  [0.0, 0.0, 0.0, 0.0],       # a conf that is not > 0: bin 0 of class 0
                  [0.1, 0.2, 0.3, 0.4375]], f32)
    pred, cbin, labels = R.pseudo_ref(p, 16, tbin=[7, 8, 16, 0], ignore_index=255)
    assert pred.tolist() == [1, 0, 1, 2, 0, 3]
    assert cbin.tolist() == [8, 6, 0, 15, 0, 7]
    # class 1 at its threshold is kept, class 0 below 7 is not, NaN class 1 in bin 0 is not, class 2
    # at tbin = bins keeps nothing, class 0 bin 0 is not kept, class 3 at tbin 0 keeps all
    assert labels.tolist() == [1, 255, 255, 255, 255, 3]
    pred2, cbin2, none = R.pseudo_ref(p.reshape(2, 3, 4), 16)
    assert none is None and pred2.shape == (2, 3) and pred2.dtype == np.uint8 and cbin2.dtype == np.uint16


def test_decay_schedule():
    want = {0: 0.0, 1: 0.5, 99: 0.99, 100: 0.99}
    for updates, d in want.items():
        assert R.decay_ref(0.99, updates) == pytest.approx(d, abs=1e-15)
        assert ema.decay_schedule(0.99, updates) == R.decay_ref(0.99, updates)
        assert ema.ema_weight(0.99, updates) == R.weight_ref(0.99, updates)
        assert ema.decay_schedule(0.99, updates, warmup=False) == 0.99
    assert ema.decay_schedule(0.99, 98) == 1.0 - 1.0 / 99 < 0.99  # still warming up
    assert ema.ema_weight(0.99, 0) == 1.0 and ema.ema_weight(0.99, 1) == 0.5
    assert ema.ema_weight(0.99, 1000) == float(f32(1.0 - 0.99))  # fp32-rounded on the host
    assert R.tbin_ref(0.968, 1024) == 992 and R.tbin_ref(0.5, 16) == 8 and R.tbin_ref(0.0, 16) == 0


# ----------------------------------------------------------------------------- binding
def test_bindings_and_abi():
    assert _lib.ABI_VERSION >= 16
    for name, nargs in (("rtsds_ema_step", 6), ("rtsds_ema_many", 6), ("rtsds_upsample_pseudo", 17)):
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_int and len(args) == nargs
        assert getattr(_lib.load(), name)
    import rtsds_amd
    assert rtsds_amd.EMATeacher is ema.EMATeacher and "TeacherLoader" in selftrain.__all__


def test_entries_refuse_bad_arguments_on_the_host():
    """Shape / pointer guards return before any launch, so they can be called without a device."""
    lib = _lib.load()
    assert lib.rtsds_ema_step(None, None, None, 0, 0.5, None) == 1          # n <= 0: shape
    assert lib.rtsds_ema_step(None, None, None, 8, 0.5, None) == 2          # null pointers: unsupported
    assert lib.rtsds_ema_many(0, None, None, None, 0.5, None) == 1          # count <= 0: shape
    up = lambda c, bins: lib.rtsds_upsample_pseudo(None, None, None, None, None, 1, 2, 2, c, 4, 4, 0.5, 0.5, bins,  # noqa: E731
                                                   19, 0, None)
    assert up(1, 1024) == 1 and up(33, 1024) == 1                             # c outside [2, 32]
    assert up(19, 48) == 1 and up(19, 8) == 1 and up(19, 2048) == 1           # bins
    assert up(19, 1024) == 2                                                  # no input / no output


# ----------------------------------------------------------------------------- argument checks
def test_functional_refuses_cpu_tensors():
    x = torch.zeros(1, 19, 4, 8)
    geo = F.upsample_geometry(x, size=(32, 64))
    with pytest.raises(RuntimeError, match="HIP"):
        F.upsample_pseudo(x, geo)
    with pytest.raises(RuntimeError, match="HIP"):
        F.ema_step(torch.zeros(8), torch.zeros(8), 0.5)
    with pytest.raises(RuntimeError, match="HIP"):
        F.EmaTable([(torch.zeros(8), torch.zeros(8))])
    with pytest.raises(RuntimeError, match="EmaTable"):
        F.ema_many([(torch.zeros(8), torch.zeros(8))], 0.5)


def test_teacher_loader_argument_checks():
    with pytest.raises(RuntimeError, match="bins"):
        selftrain.TeacherLoader([], None, ignore_index=19, bins=48)
    with pytest.raises(RuntimeError, match="threshold"):
        selftrain.TeacherLoader([], None, threshold=1.5, ignore_index=19)
    with pytest.raises(RuntimeError, match="ignore_index"):
        selftrain.TeacherLoader([], None)
    ld = selftrain.TeacherLoader([0, 1, 2], None, threshold=0.968, ignore_index=19)
    assert len(ld) == 3 and ld.tbin_value == 992 and ld.bins == 1024


# ----------------------------------------------------------------------------- config
OFFLINE = {"rounds": 2, "epochs": 3, "portion": 0.2, "portion_step": 0.05, "cap": 0.9, "bins": 256, "lr_scale": 0.5,
           "scales": [0.75, 1.0], "flip": True}
ONLINE = {"mode": "online", "epochs": 2, "lr_scale": 0.1, "ema_decay": 0.99, "threshold": 0.968}


def _config(block):
    return namedtuple("Config", ["training"])({"self_training": block})


def test_config_accepts_online_block():
    assert rmain.self_training_config(_config(dict(ONLINE))) == ONLINE
    assert rmain.self_training_config(_config(dict(ONLINE, mix="classmix", bins=512)))["mix"] == "classmix"
    assert rmain.ONLINE_SELF_TRAINING_KEYS == ("epochs", "lr_scale", "ema_decay", "threshold")


@pytest.mark.parametrize("key", ["epochs", "lr_scale", "ema_decay", "threshold"])
def test_config_online_missing_key_raises(key):
    block = dict(ONLINE)
    del block[key]
    with pytest.raises(RuntimeError, match=key):
        rmain.self_training_config(_config(block))


def test_config_unknown_mode_names_the_accepted_ones():
    with pytest.raises(RuntimeError, match="'offline', 'online'"):
        rmain.self_training_config(_config(dict(ONLINE, mode="mean_teacher")))
    with pytest.raises(RuntimeError, match="classmix"):
        rmain.self_training_config(_config(dict(ONLINE, mix="cutmix")))


def test_config_offline_block_parses_as_before():
    assert rmain.self_training_config(_config(dict(OFFLINE))) == OFFLINE
    assert rmain.self_training_config(_config(dict(OFFLINE, mode="offline")))["rounds"] == 2
    partial = dict(OFFLINE)
    del partial["portion_step"]
    with pytest.raises(RuntimeError, match="portion_step"):
        rmain.self_training_config(_config(partial))
    with pytest.raises(RuntimeError, match="rounds"):  # the online key set does not satisfy the offline mode
        rmain.self_training_config(_config({k: v for k, v in ONLINE.items() if k != "mode"}))
    assert rmain.SELF_TRAINING_KEYS == ("rounds", "epochs", "portion", "portion_step", "cap", "bins", "lr_scale",
                                        "scales", "flip")


def test_shipped_config_keeps_the_online_block_commented_out():
    path = rmain.__file__.replace("main.py", "config.yaml")
    assert "self_training" not in yaml.safe_load(open(path))["training"]
    text = open(path).read()
    assert "#   mode: online" in text and "#   ema_decay:" in text and "#   threshold:" in text


def test_main_online_threads_config(tmp_path, monkeypatch):
    """main --self_training with mode: online: no sweep, no thresholds; the teacher comes from
    model_loader, the target loader is wrapped unordered, `epochs` epochs of train + validation."""
    cfg = yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))
    cfg["training"]["segmentation"].update(epochs=1)
    cfg["training"]["self_training"] = dict(ONLINE, mix="classmix")
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    seen = {"train": [], "val": 0, "teacher": [], "loader": []}
    target, source = [0, 1, 2, 3], [7]
    student, t_model, opt = object(), object(), object()
    built = []

    class Crit:
        ignore_index = 19

    def model_loader(config, is_da, name):
        built.append(name)
        return (student if len(built) == 1 else t_model), opt, Crit(), {"init_lr": 1e-3, "power": 0.9}

    class Teacher:
        updates = 0

        def __init__(self, s, t, o, decay):
            seen["teacher"].append((s, t, o, decay))

    class Loader:
        kept_sum, pixels, tbin_value, bins = None, 0, 992, 1024

        def __init__(self, loader, teacher, **kw):
            seen["loader"].append((loader, teacher, kw))

        def __len__(self):
            return 4

    def boom(*a, **k):
        raise AssertionError("the offline sweep ran in online mode")

    monkeypatch.setattr(rmain, "datasets_loader", lambda config, aug: (target, [0], source))
    monkeypatch.setattr(rmain, "model_loader", model_loader)
    monkeypatch.setattr(rmain, "val", lambda **kw: seen.__setitem__("val", seen["val"] + 1))
    monkeypatch.setattr(rmain, "train", lambda **kw: seen["train"].append(kw))
    monkeypatch.setattr(rmain, "ordered_target_loader", boom)
    monkeypatch.setattr(selftrain, "generate", boom)
    monkeypatch.setattr(selftrain, "class_thresholds", boom)
    monkeypatch.setattr(selftrain, "TeacherLoader", Loader)
    monkeypatch.setattr(ema, "EMATeacher", Teacher)
    rmain.main(["--config", str(p), "--self_training", "--model", "bisenet"])
    assert built == ["bisenet", "bisenet"]
    assert seen["teacher"] == [(student, t_model, opt, 0.99)]
    (ld, teacher, kw), = seen["loader"]
    assert ld is target and isinstance(teacher, Teacher)
    assert kw == {"threshold": 0.968, "ignore_index": 19, "bins": 1024, "source_loader": source}
    st_train = seen["train"][1:]
    assert [k["epoch"] for k in st_train] == [0, 1] and seen["val"] == 1 + 2
    for k in st_train:
        assert k["model"] is student and k["optimizer"] is opt and isinstance(k["train_loader"], Loader)
        assert k["init_lr"] == 1e-3 * 0.1 and k["max_iter"] == 2 * 4
