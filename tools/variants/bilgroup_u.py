"""Variants of bilinear_fwd_group_vec_kernel's column vectors per thread (kBilGroupU)."""
import os
import re
import sys
sys.path.insert(0, os.path.dirname(__file__))
from textvariant import CSRC, build  # noqa: E402

# the definition as it stands, whatever its current value (build() wants the exact text, once)
cur = re.search(r"static constexpr auto kBilGroupU = \d+;", open(os.path.join(CSRC, "resize.hip")).read()).group(0)
for u in sys.argv[1:]:
    build(f"bilu{u}", {"resize.hip": [(cur, f"static constexpr auto kBilGroupU = {u};")]}, ["resize"])
