#!/usr/bin/env python3
"""Record the tolerances of the route-reference suites into tests/pinned/route_ref_tol.json.

For every case of tests/{bn,chan,resize}_bits_cases.py and every output of its reference
(tests/{bn,chan,resize}_route_ref.py) the tolerance is m * max(E32, U) of tests/route_compare.py: the
reference evaluated in float32 against itself in float64, or 2^-23 of the output's magnitude, times the
margin.  Everything runs on the CPU; neither the library nor a device is touched, so no tolerance can
depend on what a kernel produced.  An integer output is recorded as "exact", the output of an unsupported
case as "unwritten".

    python tools/record_route_tol.py            # write the file
    python tools/record_route_tol.py --check    # recompute; every value within a factor of 2 of the file's
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from tests import bn_bits_cases, bn_route_ref, chan_bits_cases, chan_route_ref, resize_bits_cases, resize_route_ref  # noqa: E402
from tests import route_compare as RC  # noqa: E402

UNITS = {"bn": (bn_bits_cases, bn_route_ref), "chan": (chan_bits_cases, chan_route_ref),
         "resize": (resize_bits_cases, resize_route_ref)}
UNWRITTEN = "unwritten"


def case_tolerances(cases, ref, case):
    if hasattr(ref, "supported") and not ref.supported(case):
        return {"y": UNWRITTEN}
    h = cases.host_inputs(case)
    o64, o32 = ref.reference(case, h, torch.float64), ref.reference(case, h, torch.float32)
    return {name: RC.EXACT if o.exact else RC.tolerance(o, o32[name]) for name, o in o64.items()}


def record():
    return {unit: {cid: case_tolerances(cases, ref, case) for cid, case in zip(cases.IDS, cases.CASES)}
            for unit, (cases, ref) in UNITS.items()}


def differences(new, old):
    out = []
    for unit in UNITS:
        if sorted(new[unit]) != sorted(old.get(unit, {})):
            out.append(f"{unit}: the case ids differ")
            continue
        for cid, tols in new[unit].items():
            if sorted(tols) != sorted(old[unit][cid]):
                out.append(f"{unit} {cid}: outputs {sorted(old[unit][cid])} in the file, {sorted(tols)} now")
                continue
            for name, t in tols.items():
                was = old[unit][cid][name]
                if isinstance(t, str) or isinstance(was, str):
                    if t != was:
                        out.append(f"{unit} {cid} {name}: {was!r} in the file, {t!r} now")
                elif not (was / 2 <= t <= was * 2):
                    out.append(f"{unit} {cid} {name}: {was:.3e} in the file, {t:.3e} now")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    args = ap.parse_args()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    new = record()
    if args.check:
        diffs = differences(new, RC.load_tol())
        for d in diffs:
            print(d)
        print("route_ref_tol.json:", "differs" if diffs else f"reproduced ({sum(len(v) for v in new.values())} cases)")
        return 1 if diffs else 0
    with open(RC.TOL_PATH, "w") as f:
        json.dump(new, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {RC.TOL_PATH}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
