"""A plain bench.py run end to end (its own process): --steps sets the timed steps, the result
line carries the headline fields and none of the --full legs, and --dump-outputs writes the
last step's arrays.  GPU only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_result_line_and_dump(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["ms_per_step"] > 0
    # value = images per second of the timed steps: batch 8 per step (rounded fields)
    assert abs(d["value"] * d["ms_per_step"] / 8000.0 - 1) < 1e-2
    assert abs(d["timed_s"] * 1000.0 / 3 - d["ms_per_step"]) <= 0.5
    for leg in ("cpu_baseline", "roofline", "inference_fps_bs8", "inference_fps_bs1", "inference_roofline"):
        assert leg not in d, leg
    arrays = {p.name: np.load(p) for p in out.iterdir()}
    assert sorted(arrays) == ["correct.npy", "loss.npy", "params.npy"]
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 1024 * 1024
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), name
    assert abs(float(arrays["loss.npy"][0]) - d["final_loss"]) <= 1e-4
    assert 0 <= arrays["correct.npy"][0] <= 8 * 512 * 1024
