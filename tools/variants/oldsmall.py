"""A/B variant: the round-5 serial-load loops of pooled_wgrad_kernel, colsum_part_kernel and
colsum_final_kernel (one load per iteration), taken from git REV's conv.hip (today in
conv_pooled.hip and conv_wgrad.hip): oldsmall.py [REV]."""
import os
import subprocess
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from textvariant import ROOT, build  # noqa: E402

rev = sys.argv[1] if len(sys.argv) > 1 else "c160d4a"
old = subprocess.check_output(["git", "-C", ROOT, "show", f"{rev}:rtsds_amd/csrc/conv.hip"], text=True)


def cur(unit):
    return open(os.path.join(ROOT, "rtsds_amd", "csrc", unit)).read()


def region(text, start, *ends):
    """From start up to the first of the end markers that follows it."""
    i = text.index(start)
    return text[i:min(text.index(e, i) for e in ends if e in text[i:])]


# the kernels' units today; REV holds both in conv.hip
edits = {}
for unit, a, b in (("conv_pooled.hip", "__global__ void __launch_bounds__(256) pooled_wgrad_kernel",
                    ("// ---- the FFM attention's backward", "// Vector forms (C % V == 0)")),
                   ("conv_wgrad.hip", "__global__ void __launch_bounds__(256) colsum_part_kernel", ("static const int kColsumRB",))):
    edits[unit] = [(region(cur(unit), a, *b), region(old, a, *b))]
build("oldsmall", edits, ["conv_pooled", "conv_wgrad"])
