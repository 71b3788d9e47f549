"""Class-balanced pseudo-labels, host side (no GPU): the two C entries' bindings and pre-launch
refusals, selftrain.class_thresholds on hand-written histograms, the global (all-reduced)
histogram, PseudoLabelLoader's refusals and the --self_training CLI / config plumbing."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import yaml

from rtsds_amd import _lib
from rtsds_amd import main as rmain
from rtsds_amd import selftrain

SHAPE, UNSUPPORTED = 1, 2
PTR = 1 << 20  # never dereferenced: every call below returns from the host-side checks


# ----------------------------------------------------------------------------- C ABI
def test_entries_are_bound():
    res, args = _lib.SIGNATURES["rtsds_conf_hist"]
    assert res is ctypes.c_int and len(args) == 9
    res, args = _lib.SIGNATURES["rtsds_pseudo_select"]
    assert res is ctypes.c_int and len(args) == 8
    assert _lib.ABI_VERSION >= 12
    lib = _lib.load()
    assert lib.rtsds_conf_hist and lib.rtsds_pseudo_select


def _hist_call(acc=PTR, hist=2 * PTR, pred=3 * PTR, cbin=4 * PTR, total=100, c=19, bins=1024):
    return _lib.load().rtsds_conf_hist(acc, hist, pred, cbin, total, c, bins, 1.0, None)


def _select_call(pred=PTR, cbin=2 * PTR, tbin=3 * PTR, out=4 * PTR, total=100, c=19):
    return _lib.load().rtsds_pseudo_select(pred, cbin, tbin, out, total, c, 19, None)


def test_conf_hist_rejects_bad_arguments_before_launch():
    assert _hist_call(total=0) == SHAPE
    assert _hist_call(total=-5) == SHAPE
    assert _hist_call(c=1) == SHAPE
    assert _hist_call(c=33) == SHAPE
    for bins in (0, 8, 24, 1000, 2048, -16):
        assert _hist_call(bins=bins) == SHAPE, bins
    assert _hist_call(acc=None) == UNSUPPORTED
    assert _hist_call(hist=None) == UNSUPPORTED
    # the privatised histogram plus a 512-pixel tile must fit 160 KiB of LDS:
    # c * (bins + 512) * 4 = 196608 B at 32 x 1024, 167936 B at 27 x 1024
    assert _hist_call(c=32, bins=1024) == UNSUPPORTED
    assert _hist_call(c=27, bins=1024) == UNSUPPORTED


def test_pseudo_select_rejects_bad_arguments_before_launch():
    assert _select_call(total=0) == SHAPE
    assert _select_call(c=1) == SHAPE
    assert _select_call(c=33) == SHAPE
    for name in ("pred", "cbin", "tbin", "out"):
        assert _select_call(**{name: None}) == UNSUPPORTED, name


def test_functional_guards_refuse_cpu_tensors():
    from rtsds_amd import functional as F
    acc = torch.zeros(1, 4, 4, 19)
    hist = torch.zeros(19, 16, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP"):
        F.confidence_histogram(acc, hist)
    with pytest.raises(RuntimeError, match="HIP"):
        F.pseudo_select(torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint16),
                        torch.zeros(19, dtype=torch.int32), 19)


# ----------------------------------------------------------------------------- class_thresholds
def _hist(rows, bins=16):
    h = torch.zeros(len(rows), bins, dtype=torch.int64)
    for k, row in enumerate(rows):
        for b, v in row.items():
            h[k, b] = v
    return h


def _kept(h, tbin):
    return [int(h[k, min(int(tbin[k]), h.shape[1]):].sum()) for k in range(h.shape[0])]


def test_class_thresholds_hand_written():
    h = _hist([{3: 5, 9: 10, 15: 5},      # N = 20
               {0: 7},                     # a single bin, the lowest
               {},                         # empty class
               {12: 1, 13: 1, 14: 1, 15: 1}])
    t = selftrain.class_thresholds(h, 1.0)
    assert t.dtype == torch.int32 and t.tolist() == [3, 0, 16, 12]  # lowest non-empty bin; empty -> bins
    t = selftrain.class_thresholds(h, 1e-9)
    assert t.tolist() == [15, 0, 16, 15]  # need = 1: the highest non-empty bin
    # exact boundary: need = ceil(0.25 * 20) = 5 = the top bin's population -> the top bin alone;
    # one pixel more (need = 6) has to take in bin 9
    assert selftrain.class_thresholds(h, 0.25).tolist()[0] == 15
    assert selftrain.class_thresholds(h, 0.26).tolist()[0] == 9
    assert selftrain.class_thresholds(h, 0.75).tolist()[0] == 9   # need = 15 = 5 + 10 exactly
    assert selftrain.class_thresholds(h, 0.76).tolist()[0] == 3
    assert selftrain.class_thresholds(h, 0.5).tolist()[3] == 14   # need = 2


def test_class_thresholds_cap_only_lowers():
    h = _hist([{3: 5, 9: 10, 15: 5}, {0: 7}, {}, {12: 1, 13: 1, 14: 1, 15: 1}])
    for portion in (1e-9, 0.25, 0.5, 1.0):
        free = selftrain.class_thresholds(h, portion)
        for cap in (0.25, 0.5, 0.9, 1.0):
            capped = selftrain.class_thresholds(h, portion, cap=cap)
            assert (capped <= free).all()
            assert int(capped.max()) <= int(np.floor(cap * 16))
            assert capped.tolist() == [min(int(v), int(np.floor(cap * 16))) for v in free]
    assert selftrain.class_thresholds(h, 1e-9, cap=0.5).tolist() == [8, 0, 8, 8]


def test_class_thresholds_kept_count_identity():
    g = torch.Generator().manual_seed(3)
    h = torch.randint(0, 50, (7, 64), generator=g)
    h[2] = 0
    h[:, :5] = 0
    for portion in (0.01, 0.2, 0.5, 0.999, 1.0):
        t = selftrain.class_thresholds(h, portion)
        kept = _kept(h, t)
        for k in range(7):
            n_k = int(h[k].sum())
            if n_k == 0:
                assert int(t[k]) == 64 and kept[k] == 0
                continue
            need = max(1, int(np.ceil(np.float64(portion) * n_k)))
            b = int(t[k])
            assert need <= kept[k] <= need - 1 + int(h[k, b])  # at most one bin's population beyond
            assert kept[k] - int(h[k, b]) < need               # and no higher threshold would do
        labels = selftrain.PseudoLabels(h, [], [], 64)
        frac = selftrain.kept_fraction(labels, t)
        assert np.isnan(frac[2])
        for k in (0, 1, 3, 4, 5, 6):
            assert frac[k] == kept[k] / int(h[k].sum()) and frac[k] >= portion


def test_class_thresholds_refuses_bad_arguments():
    h = _hist([{1: 1}, {2: 2}])
    for portion in (0.0, -0.1, 1.5):
        with pytest.raises(RuntimeError, match="portion"):
            selftrain.class_thresholds(h, portion)
    with pytest.raises(RuntimeError, match="cap"):
        selftrain.class_thresholds(h, 0.5, cap=0.0)
    with pytest.raises(RuntimeError, match="int64"):
        selftrain.class_thresholds(h.float(), 0.5)


# ----------------------------------------------------------------------------- global histogram
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_hist(rank):
    # rank 0 alone would put class 0's threshold at bin 10, rank 1 alone at bin 2
    return _hist([{10: 4}, {5: 1}]) if rank == 0 else _hist([{2: 12}, {}])


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from rtsds_amd.utils import init_distributed
    init_distributed("gloo")
    h = _rank_hist(rank)
    before = h.clone()
    t = selftrain.class_thresholds(h, 0.5)
    q.put((rank, t.tolist(), bool((h == before).all())))
    dist.barrier()
    dist.destroy_process_group()


def test_class_thresholds_allreduces_hist_over_ranks():
    """Two gloo ranks: both get the thresholds of the summed histogram -- [2, 5], which neither
    rank's own histogram gives (rank 0: [10, 5], rank 1: [2, 16]) -- and the caller's histogram
    is left as it was."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    want = selftrain.class_thresholds(_rank_hist(0) + _rank_hist(1), 0.5).tolist()
    assert want == [2, 5]
    assert selftrain.class_thresholds(_rank_hist(0), 0.5).tolist() == [10, 5]
    assert selftrain.class_thresholds(_rank_hist(1), 0.5).tolist() == [2, 16]
    for rank, t, untouched in res:
        assert t == want and untouched


# ----------------------------------------------------------------------------- PseudoLabelLoader
def _labels(nb, shape=(2, 8, 16), c=19, bins=16):
    return selftrain.PseudoLabels(torch.zeros(c, bins, dtype=torch.int64),
                                  [torch.zeros(shape, dtype=torch.uint8) for _ in range(nb)],
                                  [torch.zeros(shape, dtype=torch.uint16) for _ in range(nb)], bins)


def _batches(nb, shape=(2, 3, 8, 16)):
    return [(torch.zeros(shape), torch.zeros(shape[0], 1, *shape[2:], dtype=torch.int64)) for _ in range(nb)]


class _Lying:
    """A loader whose len() is not the number of batches it yields."""

    def __init__(self, data, n):
        self.data, self.n = data, n

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(self.data)


def test_pseudo_label_loader_refuses_mismatches():
    tbin = torch.zeros(19, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="batches"):
        selftrain.PseudoLabelLoader(_batches(3), _labels(2), tbin, 19)
    with pytest.raises(RuntimeError, match="batches"):  # fewer than recorded
        list(selftrain.PseudoLabelLoader(_Lying([], 2), _labels(2), tbin, 19))
    with pytest.raises(RuntimeError, match="shape"):
        list(selftrain.PseudoLabelLoader(_batches(2, (2, 3, 8, 24)), _labels(2), tbin, 19))
    with pytest.raises(RuntimeError, match="shape"):
        list(selftrain.PseudoLabelLoader(_batches(2, (1, 3, 8, 16)), _labels(2), tbin, 19))
    with pytest.raises(RuntimeError, match="thresholds"):
        selftrain.PseudoLabelLoader(_batches(2), _labels(2), torch.zeros(5, dtype=torch.int32), 19)
    loader = selftrain.PseudoLabelLoader(_batches(2), _labels(2), tbin, 19)
    assert len(loader) == 2
    loader.set_thresholds(torch.full((19,), 7, dtype=torch.int32))  # replaced without a sweep
    assert loader.tbin.tolist() == [7] * 19


# ----------------------------------------------------------------------------- CLI / config
ST = {"rounds": 2, "epochs": 3, "portion": 0.2, "portion_step": 0.05, "cap": 0.9, "bins": 256, "lr_scale": 0.5,
      "scales": [0.75, 1.0], "flip": True}


def _shipped():
    return yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))


def test_shipped_config_has_no_self_training_block():
    assert "self_training" not in _shipped()["training"]


class _Crit:
    ignore_index = 19


def _run_main(tmp_path, monkeypatch, argv, block=None, da=False):
    cfg = _shipped()
    cfg["training"]["segmentation"].update(epochs=1)
    cfg["training"]["domain_adaptation"].update(epochs=1, iterations=1)
    if block is not None:
        cfg["training"]["self_training"] = block
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    seen = {"train": [], "val": [], "generate": [], "thresholds": [], "loader": [], "order": []}
    target = [0, 1, 2, 3]  # a 4-batch "loader"
    model, opt = object(), object()
    monkeypatch.setattr(rmain, "datasets_loader", lambda config, aug: (target, [0], [0]))
    if da:
        monkeypatch.setattr(rmain, "model_loader", lambda config, is_da, name: (
            (model, opt, _Crit(), {"gen_init_lr": 1e-3, "gen_power": 0.9}),
            (object(), None, None, {"dis_init_lr": 1e-4, "dis_power": 0.9})))
        monkeypatch.setattr(rmain, "adversarial_train", lambda **kw: seen["order"].append("adversarial_train"))
        monkeypatch.setattr(rmain, "val_GTA5", lambda *a, **kw: seen["val"].append((a, kw)))
    else:
        monkeypatch.setattr(rmain, "model_loader", lambda config, is_da, name: (model, opt, _Crit(),
                                                                                {"init_lr": 1e-3, "power": 0.9}))
        monkeypatch.setattr(rmain, "val", lambda **kw: seen["val"].append(((), kw)))
    monkeypatch.setattr(rmain, "train", lambda **kw: (seen["train"].append(kw), seen["order"].append("train")))

    labels = selftrain.PseudoLabels(torch.zeros(19, ST["bins"], dtype=torch.int64), [None] * 4, [None] * 4, ST["bins"])

    def generate(m, loader, num_classes, **kw):
        seen["generate"].append(dict(kw, model=m, loader=loader, num_classes=num_classes))
        seen["order"].append("generate")
        return labels

    def thresholds(hist, portion, cap=None):
        seen["thresholds"].append((hist, portion, cap))
        return torch.zeros(19, dtype=torch.int32)

    class Loader:
        def __init__(self, loader, lab, tbin, ignore_index):
            seen["loader"].append((loader, lab, tbin, ignore_index))

    monkeypatch.setattr(selftrain, "generate", generate)
    monkeypatch.setattr(selftrain, "class_thresholds", thresholds)
    monkeypatch.setattr(selftrain, "PseudoLabelLoader", Loader)
    rmain.main(["--config", str(p)] + argv)
    return seen, model, opt, target, labels


def test_main_without_flag_never_touches_selftrain(tmp_path, monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("self-training entered without --self_training")
    monkeypatch.setattr(rmain, "self_train", boom)
    monkeypatch.setattr(rmain, "self_training_config", boom)
    # the block alone does nothing either
    seen, *_ = _run_main(tmp_path, monkeypatch, [], block=dict(ST))
    assert not seen["generate"] and not seen["thresholds"] and not seen["loader"]
    assert len(seen["train"]) == 1 and len(seen["val"]) == 1
    seen, *_ = _run_main(tmp_path, monkeypatch, ["--domain_adaptation"], block=dict(ST), da=True)
    assert not seen["generate"] and seen["order"] == ["adversarial_train"]


def test_main_self_training_threads_config_keys_seg(tmp_path, monkeypatch):
    seen, model, opt, target, labels = _run_main(tmp_path, monkeypatch, ["--self_training"], block=dict(ST))
    # the normal run first, then per round: one sweep, then `epochs` epochs
    assert seen["order"] == ["train"] + (["generate"] + ["train"] * 3) * 2
    for g in seen["generate"]:
        assert g["model"] is model and g["loader"] is target and g["num_classes"] == 19
        assert g["bins"] == 256 and tuple(g["scales"]) == (0.75, 1.0) and g["flip"] is True
    assert [(p, c) for _, p, c in seen["thresholds"]] == [(0.2, 0.9), (0.25, 0.9)]
    assert all(h is labels.hist for h, _, _ in seen["thresholds"])
    assert all(ld is target and lab is labels and ig == 19 for ld, lab, _, ig in seen["loader"])
    st_train = seen["train"][1:]
    assert [kw["epoch"] for kw in st_train] == list(range(6))
    for kw in st_train:
        assert kw["model"] is model and kw["optimizer"] is opt and isinstance(kw["criterion"], _Crit)
        assert kw["init_lr"] == 1e-3 * 0.5 and kw["max_iter"] == 2 * 3 * 4 and kw["power"] == 0.9
        assert isinstance(kw["train_loader"], selftrain.PseudoLabelLoader)
    assert len(seen["val"]) == 1 + 6  # validation after every epoch, as the branch does


def test_main_self_training_threads_config_keys_da(tmp_path, monkeypatch):
    seen, model, opt, target, labels = _run_main(tmp_path, monkeypatch, ["--self_training", "--domain_adaptation"],
                                                 block=dict(ST, rounds=1, epochs=2), da=True)
    assert seen["order"] == ["adversarial_train", "generate", "train", "train"]
    for kw in seen["train"]:  # the generator's model, optimizer and criterion
        assert kw["model"] is model and kw["optimizer"] is opt and kw["init_lr"] == 1e-3 * 0.5
        assert kw["max_iter"] == 1 * 2 * 4
    assert len(seen["val"]) == 2 and all(a[1] is model for a, _ in seen["val"])


def test_main_self_training_without_block_raises(tmp_path, monkeypatch):
    with pytest.raises(RuntimeError, match="training.self_training"):
        _run_main(tmp_path, monkeypatch, ["--self_training"])
    partial = dict(ST)
    del partial["portion_step"]
    with pytest.raises(RuntimeError, match="portion_step"):
        _run_main(tmp_path, monkeypatch, ["--self_training"], block=partial)
