#!/bin/bash
# One full bench line per workload -> $OUT_DIR/<tag>_bench_<workload>.json (+ .log); OUT_DIR defaults to bench_out
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
out=${OUT_DIR:-bench_out}; mkdir -p "$out"
tag=$1; shift
wls=${@:-bisenet-seg bisenet-da deeplab-seg deeplab-da}
for wl in $wls; do
  timeout -k 10 600 python3 -u bench.py --full --workload $wl > $out/${tag}_bench_$wl.json 2> $out/${tag}_bench_$wl.log
  cat $out/${tag}_bench_$wl.json
done
