"""bench.py's command line and its --dump-outputs writer, on the CPU (no kernels run)."""
import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    args = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (args.gpus, args.steps, args.warmup) == (1, 7, 2)
    assert args.full is False and args.dump_outputs is None
    args = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert args.full is True and args.dump_outputs == "d"


def test_conv_report_needs_full(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--conv-report")
    assert _parse(monkeypatch, "--full", "--conv-report").conv_report


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_every_array(tmp_path, monkeypatch):
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy()
    loss, corr = torch.tensor(2.5), torch.tensor([12345], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "a"), loss, corr, net)
    got = {p.name: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["correct.npy", "loss.npy", "params.npy"]
    assert got["loss.npy"].dtype == np.float64 and got["loss.npy"].tolist() == [2.5]
    assert got["correct.npy"].dtype == np.float64 and got["correct.npy"].tolist() == [12345.0]
    assert got["params.npy"].dtype == np.float32
    np.testing.assert_array_equal(got["params.npy"], flat)

    # more parameters than the cap: a fixed sample of positions, in order, the same every time
    monkeypatch.setattr(bench, "DUMP_PARAM_ELEMS", 16)
    bench.dump_outputs(str(tmp_path / "b"), loss, corr, net)
    bench.dump_outputs(str(tmp_path / "c"), loss, corr, net)
    b, c = np.load(tmp_path / "b" / "params.npy"), np.load(tmp_path / "c" / "params.npy")
    assert b.shape == (16,)
    np.testing.assert_array_equal(b, c)
    pos, i = [], 0
    for v in b:  # b is a subsequence of flat
        while flat[i] != v:
            i += 1
        pos.append(i)
        i += 1
    assert len(pos) == 16 and pos[-1] < flat.size
