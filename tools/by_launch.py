"""A rocprofv3 kernel_trace.csv grouped by kernel instantiation and grid size: mean duration,
launches per step and their product, largest first; then the total launches per step.
usage: by_launch.py <run_kernel_trace.csv> STEPS [name-substring ...]   (substrings: only those kernels)"""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
steps = float(sys.argv[2])
only = sys.argv[3:]
agg = collections.defaultdict(lambda: [0, 0.0])
for r in rows:
    name = r["Kernel_Name"]
    if only and not any(s in name for s in only):
        continue
    grid = r.get("Grid_Size", r.get("Grid_Size_X", "?"))
    wg = r.get("Workgroup_Size", r.get("Workgroup_Size_X", "?"))
    a = agg[(name, grid, wg)]
    a[0] += 1
    a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
for (name, grid, wg), (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
    print(f"{t / n / 1e3:9.1f} us  x {n / steps:6.2f}/step  = {t / steps / 1e3:8.1f} us/step  grid {grid:>9} wg {wg:>4}  {name[:110]}")
print(f"launches per step: {sum(n for n, _ in agg.values()) / steps:.1f}   "
      f"kernel us per step: {sum(t for _, t in agg.values()) / steps / 1e3:.1f}")
