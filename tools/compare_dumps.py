"""Compare two directories written by ``bench.py --dump-outputs``: every array bit for bit.

    python tools/compare_dumps.py DIR_A DIR_B      # exit status 1 when any array differs
"""
import os
import sys

import numpy as np


def main(a, b):
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b)), (names, sorted(os.listdir(b)))
    bad = [n for n in names if np.load(os.path.join(a, n)).tobytes() != np.load(os.path.join(b, n)).tobytes()]
    print(f"{len(names)} dumped arrays, {len(names) - len(bad)} bit-equal, differing: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
