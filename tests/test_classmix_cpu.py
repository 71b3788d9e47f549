"""ClassMix, host side (no GPU): the two C entries' bindings and pre-launch refusals, the
functional wrappers' refusal of CPU tensors, the numpy reference (tests/classmix_ref.py) on
hand-written cases, ClassMixLoader's refusals and the training.self_training.mix plumbing."""
import ctypes

import numpy as np
import pytest
import torch
import yaml

from rtsds_amd import _lib
from rtsds_amd import main as rmain
from rtsds_amd import selftrain
from tests import classmix_ref as R

SHAPE, UNSUPPORTED = 1, 2
PTR = 1 << 20  # never dereferenced: every call below returns from the host-side checks


# ----------------------------------------------------------------------------- C ABI
def test_entries_are_bound():
    res, args = _lib.SIGNATURES["rtsds_class_presence"]
    assert res is ctypes.c_int and len(args) == 11
    res, args = _lib.SIGNATURES["rtsds_classmix"]
    assert res is ctypes.c_int and len(args) == 24
    assert _lib.ABI_VERSION >= 14
    lib = _lib.load()
    assert lib.rtsds_class_presence and lib.rtsds_classmix


def _presence_call(slab=PTR, origins=2 * PTR, pitch=2, present=3 * PTR, n=2, hs=37, ws=333, h=24, w=300, c=19):
    return _lib.load().rtsds_class_presence(slab, origins, pitch, present, n, hs, ws, h, w, c, None)


MIX_PTRS = ("src", "slab", "tgt", "pred", "cbin", "tbin", "present", "perm", "origins", "out_img", "out_lab", "mask",
            "chosen")


def _mix_call(n=2, hs=37, ws=333, h=24, w=300, c=19, pix=8, ppitch=None, opitch=2, **ptrs):
    p = {name: (i + 1) * PTR for i, name in enumerate(MIX_PTRS)}
    p.update(ptrs)
    return _lib.load().rtsds_classmix(p["src"], p["slab"], p["tgt"], p["pred"], p["cbin"], p["tbin"], p["present"],
                                      p["perm"], c if ppitch is None else ppitch, p["origins"], opitch, p["out_img"],
                                      p["out_lab"], p["mask"], p["chosen"], n, hs, ws, h, w, c, pix, 19, None)


def test_class_presence_rejects_bad_arguments_before_launch():
    for name in ("slab", "origins", "present"):
        assert _presence_call(**{name: None}) == UNSUPPORTED, name
    assert _presence_call(slab=PTR + 4) == UNSUPPORTED      # int64 labels off an 8-byte boundary
    assert _presence_call(origins=PTR + 2) == UNSUPPORTED
    assert _presence_call(c=1) == SHAPE
    assert _presence_call(c=33) == SHAPE
    assert _presence_call(h=0) == SHAPE and _presence_call(w=0) == SHAPE  # a zero-sized window
    assert _presence_call(n=0) == SHAPE
    assert _presence_call(h=38) == SHAPE and _presence_call(w=334) == SHAPE  # a window outside the source
    assert _presence_call(pitch=1) == SHAPE


def test_classmix_rejects_bad_arguments_before_launch():
    for name in MIX_PTRS[:11]:  # mask and chosen are optional
        assert _mix_call(**{name: None}) == UNSUPPORTED, name
    assert _mix_call(c=1) == SHAPE
    assert _mix_call(c=33) == SHAPE
    assert _mix_call(pix=7) == UNSUPPORTED
    for pix in (0, 4, 10, 24):
        assert _mix_call(pix=pix) == UNSUPPORTED, pix
    assert _mix_call(h=0) == SHAPE and _mix_call(w=0) == SHAPE
    assert _mix_call(h=38) == SHAPE and _mix_call(w=334) == SHAPE
    assert _mix_call(n=0) == SHAPE
    assert _mix_call(ppitch=18) == SHAPE and _mix_call(opitch=1) == SHAPE
    assert _mix_call(slab=PTR + 4) == UNSUPPORTED and _mix_call(out_lab=PTR + 4) == UNSUPPORTED
    assert _mix_call(cbin=PTR + 1) == UNSUPPORTED and _mix_call(perm=PTR + 2) == UNSUPPORTED
    assert _mix_call(pix=8, src=PTR + 4) == UNSUPPORTED   # an 8-byte record off its alignment
    assert _mix_call(pix=16, tgt=PTR + 8) == UNSUPPORTED
    assert _mix_call(pix=6, out_img=PTR + 1) == UNSUPPORTED


def test_functional_guards_refuse_cpu_tensors():
    from rtsds_amd import functional as F
    slab = torch.zeros(1, 8, 8, dtype=torch.int64)
    origins = torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.class_presence(slab, (4, 4), origins)
    img = torch.zeros(1, 3, 8, 8).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.classmix(img, slab, img[:, :, :4, :4], torch.zeros(1, 4, 4, dtype=torch.uint8),
                   torch.zeros(1, 4, 4, dtype=torch.uint16), torch.zeros(19, dtype=torch.int32),
                   torch.zeros(1, 19, dtype=torch.int32), origins, 19)


# ----------------------------------------------------------------------------- the reference
def _lab(rows):
    return np.array(rows, dtype=np.int64)[None]


def test_reference_three_present_choose_two_smallest_keys():
    slab = _lab([[4, 4, 9], [9, 17, 17]])
    assert R.presence(slab, (2, 3), [(0, 0)], 19)[0] == (1 << 4) | (1 << 9) | (1 << 17)
    perm = list(range(19))
    perm[4], perm[9], perm[17] = 12, 3, 7
    assert R.choose((1 << 4) | (1 << 9) | (1 << 17), perm, 19) == (1 << 9) | (1 << 17)  # m = 2: keys 3 and 7
    perm[4] = 0  # keys of classes that are absent do not count
    perm[0] = -5
    assert R.choose((1 << 4) | (1 << 9) | (1 << 17), perm, 19) == (1 << 4) | (1 << 9)
    # the window, not the map: a window holding only the last column sees two classes
    assert R.presence(slab, (2, 1), [(0, 2)], 19)[0] == (1 << 9) | (1 << 17)


def test_reference_equal_keys_break_to_lower_class():
    p = (1 << 2) | (1 << 5) | (1 << 11) | (1 << 12)
    assert R.choose(p, [7] * 19, 19) == (1 << 2) | (1 << 5)  # m = 2 of 4, all keys equal
    keys = [7] * 19
    keys[12] = 1
    assert R.choose(p, keys, 19) == (1 << 12) | (1 << 2)


def test_reference_class_31_alone_and_empty():
    slab = np.full((1, 3, 3), 31, dtype=np.int64)
    pr = R.presence(slab, (3, 3), [(0, 0)], 32)
    assert pr.dtype == np.uint32 and int(pr[0]) == 1 << 31    # the sign bit of an int32
    assert R.choose(pr[0], list(range(32)), 32) == 1 << 31    # a single class: m = 1, it is chosen
    assert int(R.presence(slab, (3, 3), [(0, 0)], 19)[0]) == 0  # 31 is no class of 19
    for v in (-100, 255, 19, 24):
        assert int(R.presence(np.full((1, 2, 2), v, dtype=np.int64), (2, 2), [(0, 0)], 19)[0]) == 0
    assert R.choose(0, list(range(19)), 19) == 0               # present == 0 -> chosen == 0


def test_reference_mix_small_case():
    c, ignore = 3, 9
    slab = _lab([[0, 1, 2, -100], [1, 1, 3, 3]])  # class 0 lies outside the window
    src = np.arange(1 * 2 * 4 * 6, dtype=np.uint8).reshape(1, 2, 4, 6)
    tgt = (200 + np.arange(1 * 2 * 3 * 6)).astype(np.uint8).reshape(1, 2, 3, 6)
    pred = np.array([[[0, 2, 5], [1, 1, 2]]], dtype=np.uint8)
    cbin = np.array([[[4, 4, 4], [9, 2, 5]]], dtype=np.uint16)
    tbin = [5, 3, 4]
    perm = np.array([[2, 0, 1]])  # of the present {1, 2} (window x0 = 1): class 1 has the smaller key
    r = R.classmix(src, slab, tgt, pred, cbin, tbin, perm, [(0, 1)], ignore)
    assert int(r["present"][0]) == 0b110 and int(r["chosen"][0]) == 0b010
    assert r["mask"].tolist() == [[[1, 0, 0], [1, 0, 0]]]
    # target side: pred 2 / bin 4 >= 4 kept; pred 5 is no class; pred 1 / bin 2 < 3; pred 2 / bin 5 kept
    assert r["out_lab"].tolist() == [[[1, 2, ignore], [1, ignore, 2]]]
    assert np.array_equal(r["out_img"][0, 0, 0], src[0, 0, 1]) and np.array_equal(r["out_img"][0, 1, 0], src[0, 1, 1])
    assert np.array_equal(r["out_img"][0, :, 1:], tgt[0, :, 1:])


# ----------------------------------------------------------------------------- ClassMixLoader
def _labels(nb, shape=(2, 8, 16), c=19, bins=16):
    return selftrain.PseudoLabels(torch.zeros(c, bins, dtype=torch.int64),
                                  [torch.zeros(shape, dtype=torch.uint8) for _ in range(nb)],
                                  [torch.zeros(shape, dtype=torch.uint16) for _ in range(nb)], bins)


def _batches(nb, shape=(2, 3, 8, 16)):
    return [(torch.zeros(shape), torch.zeros(shape[0], 1, *shape[2:], dtype=torch.int64)) for _ in range(nb)]


def test_classmix_loader_refuses_mismatches():
    tbin = torch.zeros(19, dtype=torch.int32)
    src = _batches(2, (2, 3, 10, 20))
    with pytest.raises(RuntimeError, match="batches"):
        selftrain.ClassMixLoader(_batches(3), src, _labels(2), tbin, 19)
    with pytest.raises(RuntimeError, match="thresholds"):
        selftrain.ClassMixLoader(_batches(2), src, _labels(2), torch.zeros(5, dtype=torch.int32), 19)
    with pytest.raises(RuntimeError, match="shape"):
        list(selftrain.ClassMixLoader(_batches(2, (2, 3, 8, 24)), src, _labels(2), tbin, 19))
    for small in ((1, 3, 10, 20), (2, 3, 7, 20), (2, 3, 10, 15)):  # fewer samples, lower, narrower
        with pytest.raises(RuntimeError, match="smaller"):
            list(selftrain.ClassMixLoader(_batches(2), _batches(2, small), _labels(2), tbin, 19))
    with pytest.raises(RuntimeError, match="no batch"):
        list(selftrain.ClassMixLoader(_batches(2), [], _labels(2), tbin, 19))
    loader = selftrain.ClassMixLoader(_batches(2), src, _labels(2), tbin, 19)
    assert isinstance(loader, selftrain.PseudoLabelLoader) and len(loader) == 2 and loader.last_chosen is None
    loader.set_thresholds(torch.full((19,), 7, dtype=torch.int32))
    assert loader.tbin.tolist() == [7] * 19


def test_classmix_loader_restarts_a_short_source_loader():
    class Counting:
        def __init__(self, data):
            self.data, self.iters = data, 0

        def __iter__(self):
            self.iters += 1
            return iter(self.data)

    src = Counting(_batches(2, (2, 3, 10, 20)))
    loader = selftrain.ClassMixLoader(_batches(2), src, _labels(2), torch.zeros(19, dtype=torch.int32), 19)
    got = [loader._next_source() for _ in range(5)]
    assert [g[0] is src.data[i % 2][0] for i, g in enumerate(got)] == [True] * 5
    assert src.iters == 3


def test_classmix_loader_draw_order():
    """Per sample, in order: y0, x0, perm -- from torch's default CPU generator."""
    torch.manual_seed(11)
    blk = selftrain.ClassMixLoader.draw(3, 19, 80, 160, 64, 128)
    assert blk.dtype == torch.int32 and tuple(blk.shape) == (3, 21)
    torch.manual_seed(11)
    for i in range(3):
        assert int(blk[i, 0]) == int(torch.randint(0, 17, (1,)))
        assert int(blk[i, 1]) == int(torch.randint(0, 33, (1,)))
        assert blk[i, 2:].tolist() == torch.randperm(19).tolist()
    same = selftrain.ClassMixLoader.draw(2, 5, 8, 8, 8, 8)  # source = target size: the only origin is (0, 0)
    assert same[:, :2].tolist() == [[0, 0], [0, 0]] and sorted(same[0, 2:].tolist()) == list(range(5))


# ----------------------------------------------------------------------------- CLI / config
ST = {"rounds": 2, "epochs": 1, "portion": 0.2, "portion_step": 0.05, "cap": 0.9, "bins": 256, "lr_scale": 0.5,
      "scales": [1.0], "flip": False}


class _Crit:
    ignore_index = 19


def _run_main(tmp_path, monkeypatch, argv, block, da=False):
    cfg = yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))
    cfg["training"]["segmentation"].update(epochs=1)
    cfg["training"]["domain_adaptation"].update(epochs=1, iterations=1)
    cfg["training"]["self_training"] = block
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    seen = {"pseudo": [], "classmix": [], "train": []}
    target, val_l, source = [0, 1, 2, 3], [0], [7, 8]
    model, opt = object(), object()
    monkeypatch.setattr(rmain, "datasets_loader", lambda config, aug: (target, val_l, source))
    if da:
        monkeypatch.setattr(rmain, "model_loader", lambda config, is_da, name: (
            (model, opt, _Crit(), {"gen_init_lr": 1e-3, "gen_power": 0.9}),
            (object(), None, None, {"dis_init_lr": 1e-4, "dis_power": 0.9})))
        monkeypatch.setattr(rmain, "adversarial_train", lambda **kw: None)
        monkeypatch.setattr(rmain, "val_GTA5", lambda *a, **kw: None)
    else:
        monkeypatch.setattr(rmain, "model_loader", lambda config, is_da, name: (model, opt, _Crit(),
                                                                                {"init_lr": 1e-3, "power": 0.9}))
        monkeypatch.setattr(rmain, "val", lambda **kw: None)
    monkeypatch.setattr(rmain, "train", lambda **kw: seen["train"].append(kw["train_loader"]))
    labels = selftrain.PseudoLabels(torch.zeros(19, ST["bins"], dtype=torch.int64), [None] * 4, [None] * 4, ST["bins"])
    tbin = torch.zeros(19, dtype=torch.int32)
    monkeypatch.setattr(selftrain, "generate", lambda m, loader, num_classes, **kw: labels)
    monkeypatch.setattr(selftrain, "class_thresholds", lambda hist, portion, cap=None: tbin)

    class Pseudo:
        def __init__(self, *args, **kwargs):
            seen["pseudo"].append((args, kwargs))

    class Mix:
        def __init__(self, *args, **kwargs):
            seen["classmix"].append((args, kwargs))

    monkeypatch.setattr(selftrain, "PseudoLabelLoader", Pseudo)
    monkeypatch.setattr(selftrain, "ClassMixLoader", Mix)
    rmain.main(["--config", str(p)] + argv)
    return seen, target, source, labels, tbin


@pytest.mark.parametrize("da", [False, True], ids=["seg", "da"])
def test_main_mix_classmix_builds_the_classmix_loader(tmp_path, monkeypatch, da):
    argv = ["--self_training"] + (["--domain_adaptation"] if da else [])
    seen, target, source, labels, tbin = _run_main(tmp_path, monkeypatch, argv, dict(ST, mix="classmix"), da=da)
    assert not seen["pseudo"] and len(seen["classmix"]) == 2  # one per round
    for args, kwargs in seen["classmix"]:
        assert not kwargs and len(args) == 5
        assert args[0] is target and args[1] is source and args[2] is labels and args[3] is tbin and args[4] == 19
    st_loaders = seen["train"][0 if da else 1:]
    assert len(st_loaders) == 2 and all(isinstance(ld, selftrain.ClassMixLoader) for ld in st_loaders)


@pytest.mark.parametrize("da", [False, True], ids=["seg", "da"])
def test_main_without_mix_builds_the_pseudo_label_loader_as_before(tmp_path, monkeypatch, da):
    argv = ["--self_training"] + (["--domain_adaptation"] if da else [])
    seen, target, source, labels, tbin = _run_main(tmp_path, monkeypatch, argv, dict(ST), da=da)
    assert not seen["classmix"] and len(seen["pseudo"]) == 2
    for args, kwargs in seen["pseudo"]:
        assert not kwargs and len(args) == 4
        assert args[0] is target and args[1] is labels and args[2] is tbin and args[3] == 19


def test_main_other_mix_value_raises(tmp_path, monkeypatch):
    for value in ("other", "cutmix", True, ""):
        with pytest.raises(RuntimeError, match="mix"):
            _run_main(tmp_path, monkeypatch, ["--self_training"], dict(ST, mix=value))


def test_self_train_with_mix_needs_the_source_loader(monkeypatch):
    cfg = rmain.load_config(rmain.__file__.replace("main.py", "config.yaml"))
    with pytest.raises(RuntimeError, match="source"):
        rmain.self_train(cfg, dict(ST, mix="classmix"), object(), object(), _Crit(), 1e-3, 0.9, 1, 19, [0], None, [])


def test_mix_is_optional_and_documented_in_the_shipped_config():
    assert "mix" not in rmain.SELF_TRAINING_KEYS
    text = open(rmain.__file__.replace("main.py", "config.yaml")).read()
    assert "#   mix: classmix" in text
    shipped = yaml.safe_load(text)
    assert "self_training" not in shipped["training"]
