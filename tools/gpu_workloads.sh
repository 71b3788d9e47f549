#!/bin/bash
# One full bench line per BASELINE.json workload (1 GPU) -> $OUT_DIR/wl_<tag>_<workload>.json; OUT_DIR defaults to bench_out
set -e
cd "$GRAFT_REPO_ROOT"
out=${OUT_DIR:-bench_out}; mkdir -p "$out"
tag=${1:-r1}
for wl in bisenet-da deeplab-seg deeplab-da; do
  timeout -k 10 400 python -u bench.py --full --workload $wl --steps ${2:-10} --warmup 3 --no-cpu-baseline > $out/wl_${tag}_$wl.json 2> $out/wl_${tag}_$wl.err
done
echo done
