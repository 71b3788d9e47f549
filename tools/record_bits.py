"""Records tests/pinned/UNIT_bits.json (UNIT = bn, resize, chan): one SHA-256 per output tensor per
case of tests/UNIT_bits_cases.py, from the library this checkout built (or RTSDS_LIB).

    python tools/record_bits.py UNIT [--check] [--out FILE]
    python tools/record_bn_bits.py [--check] [--out FILE]        (UNIT = bn)
    python tools/record_resize_bits.py [--check] [--out FILE]    (UNIT = resize)
    python tools/record_chan_bits.py [--check] [--out FILE]      (UNIT = chan)

The file is recorded on the parent of a commit that means to change the unit's arithmetic --
first with --check (compares, writes nothing) to show that the committed file was still green
there -- never from the code under test.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(unit=None):
    ap = argparse.ArgumentParser()
    if unit is None:
        ap.add_argument("unit", choices=("bn", "resize", "chan"))
    ap.add_argument("--check", action="store_true", help="compare with the recorded file instead of writing it")
    ap.add_argument("--out")
    args = ap.parse_args()
    unit = unit or args.unit
    args.out = args.out or os.path.join(ROOT, "tests", "pinned", unit + "_bits.json")
    cases = importlib.import_module(f"tests.{unit}_bits_cases")
    got = {i: cases.run_case(c) for i, c in zip(cases.IDS, cases.CASES)}
    if args.check:
        with open(args.out) as f:
            want = json.load(f)
        bad = sorted(i for i in set(got) | set(want) if got.get(i) != want.get(i))
        for i in bad:
            print("differs:", i)
        print(f"{len(got) - len(bad)} of {len(got)} cases match {args.out}")
        return 1 if bad else 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(got)} cases, {sum(len(v) for v in got.values())} digests -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
