"""The channel-vector unit's bits, pinned: every output of every route of rtsds_amd/csrc/chan.hip
hashes to what tests/pinned/chan_bits.json records (tests/chan_bits_cases.py has the cases and the
driver).  The file changes only in a commit that means to change the unit's arithmetic, after
tools/record_chan_bits.py --check has shown it still green on that commit's parent."""
import json
import os

import pytest

from .chan_bits_cases import CASES, IDS, run_case

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "pinned", "chan_bits.json")) as f:
    PINNED = json.load(f)


def test_every_case_is_pinned():
    assert sorted(PINNED) == sorted(IDS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chan_bits(case):
    want = PINNED[IDS[CASES.index(case)]]
    got = run_case(case)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
