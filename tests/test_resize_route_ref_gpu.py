"""Every pinned resize route (tests/resize_bits_cases.py, the case table of tests/test_resize_bits_gpu.py) against
the float64 statement of its operation in tests/resize_route_ref.py.  The pins show that a refactor changed no
bit; this suite shows that the bits were right.  Each case runs the pin driver's launches
(run_case_outputs: same inputs, same sentinels), then the reference on the host inputs, then compares every
output within the tolerance recorded on the CPU in tests/pinned/route_ref_tol.json (tests/route_compare.py:
m * max(fp32 restatement error, 2^-23 magnitude), plus 2^-8 |ref| per element of a bf16 output; integer
outputs exactly).  No tolerance here comes from a kernel.
The scaled downsample returns RTSDS_ERR_UNSUPPORTED: it has no reference, its output must be untouched.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from tests import resize_route_ref as R  # noqa: E402
from tests import route_compare as RC  # noqa: E402
from tests.resize_bits_cases import CASES, IDS, case_id, run_case_outputs  # noqa: E402

TOL = RC.load_tol()["resize"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_route_against_float64(case):
    cid = case_id(case)
    tols = TOL[cid]
    inputs, got, rcs = run_case_outputs(case)
    if not R.supported(case):
        assert rcs[0] != 0 and RC.unwritten(got["y"]), f"{cid}: return code {rcs[0]}"
        return
    assert not any(rcs), f"{cid}: return codes {rcs}"
    ratios = RC.check_case(cid, R.reference(case, inputs, torch.float64, tols, got), got, tols)
    print(f"{cid}: worst error / allowance " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
