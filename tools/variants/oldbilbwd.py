"""A/B variant: the fused bilinear backward as of round 5 (one load per tap over the whole
table row, margins included), taken from git revision REV's ew.hip (the unit that held the
bilinear kernels before resize.hip) and patched into resize.hip: oldbilbwd.py [REV [BASE]].

The round-5 text launches the two-pass kernels under the names they had until resize.hip's
copies were folded, so it is patched into BASE's resize.hip (default: the last revision before
the fold, whose outputs are bit-identical to today's) and that file replaces the unit."""
import os
import subprocess
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from textvariant import ROOT, build  # noqa: E402

rev = sys.argv[1] if len(sys.argv) > 1 else "1bc3f56"
base = sys.argv[2] if len(sys.argv) > 2 else "e96d508"


def show(r, unit):
    return subprocess.check_output(["git", "-C", ROOT, "show", f"{r}:rtsds_amd/csrc/{unit}.hip"], text=True)


old_src, base_src = show(rev, "ew"), show(base, "resize")
cur_src = open(os.path.join(ROOT, "rtsds_amd", "csrc", "resize.hip")).read()
A, B = "// Both passes in one kernel for 16-B channel vectors", "extern \"C\" int rtsds_bilinear_fwd("


def region(text, a=A):
    i, j = text.index(a), text.index(B)
    return text[i:j]


patched = base_src.replace(region(base_src, "// [first, last] nonzero entry"), region(old_src))
build("oldbilbwd", {"resize.hip": [(cur_src, patched)]}, ["resize"])
