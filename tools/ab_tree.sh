#!/bin/bash
# Whole-step A/B of Python-level changes on one box: the tree vs an older revision's Python
# (unpacked here by: git archive REV rtsds_amd bench.py | tar -x -C _abtree) running on the
# tree's library.  usage: ab_tree.sh ROUNDS   -> per run: variant, img/s, ms/step, FPS bs 8, bs 1
# Outputs under $OUT_DIR (default bench_out).  A revision from before bench.py had --full
# measures inference without it: run with OLD_ARGS="" then.
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root"
out=$root/${OUT_DIR:-bench_out}; mkdir -p "$out"
old_args=${OLD_ARGS-"--full"}
rounds=$1
for r in $(seq 1 $rounds); do
  for v in tree old; do
    d=.; extra=--full; [ "$v" = old ] && d=_abtree && extra=$old_args
    (cd $d && RTSDS_LIB=$root/rtsds_amd/librtsds_hip.so timeout -k 10 300 python3 bench.py $extra --no-cpu-baseline --no-conv-profile) > $out/abt_$v.json 2>/dev/null || exit 1
    python3 -c "import json,sys; d=json.loads(open(sys.argv[1]).readline()); print(sys.argv[2], d['value'], d['ms_per_step'], d.get('inference_fps_bs8'), d.get('inference_fps_bs1'), flush=True)" $out/abt_$v.json $v
  done
done
