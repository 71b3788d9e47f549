"""Every pinned BatchNorm route (tests/bn_bits_cases.py, the case table of tests/test_bn_bits_gpu.py) against
the float64 statement of its operation in tests/bn_route_ref.py.  The pins show that a refactor changed no
bit; this suite shows that the bits were right.  Each case runs the pin driver's launches
(run_case_outputs: same inputs, same sentinels), then the reference on the host inputs, then compares every
output within the tolerance recorded on the CPU in tests/pinned/route_ref_tol.json (tests/route_compare.py:
m * max(fp32 restatement error, 2^-23 magnitude), plus 2^-8 |ref| per element of a bf16 output; integer
outputs exactly).  No tolerance here comes from a kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from tests import bn_route_ref as R  # noqa: E402
from tests import route_compare as RC  # noqa: E402
from tests.bn_bits_cases import CASES, IDS, case_id, run_case_outputs  # noqa: E402

TOL = RC.load_tol()["bn"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_route_against_float64(case):
    cid = case_id(case)
    tols = TOL[cid]
    inputs, got, rcs = run_case_outputs(case)
    assert not any(rcs)
    ratios = RC.check_case(cid, R.reference(case, inputs, torch.float64, tols, got), got, tols)
    print(f"{cid}: worst error / allowance " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
