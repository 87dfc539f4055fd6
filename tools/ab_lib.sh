#!/bin/bash
# GPU box: alternating bench runs of two builds of the library on the same box:  bash tools/ab_lib.sh ab/base.so "" [rounds] [tag]
#   ("" = the shipped library); per-layer CSVs of both at the end -> out/<tag>/
A=$1; B=$2; R=${3:-2}; TAG=${4:-ab_lib}
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; O=$ROOT/out/$TAG; mkdir -p $O
for i in $(seq $R); do for v in "$A" "$B"; do
  CANONSWAP_LIB=$v timeout 600 python bench.py --full --steps 10 --warmup 3 --no-fixed-job --no-cpu-baseline --no-chain --no-single-frame > $O/b.json 2>$O/b.err
  python - <<PY | tee -a $O/ab.txt
import json
try:
    d=json.loads(open("$O/b.json").read().strip().splitlines()[-1]); print("lib=[$v]", d["value"], d["roofline"]["frac"], d["ms_per_step"])
except Exception as e: print("lib=[$v] failed", e, open("$O/b.err").read()[-800:])
PY
done; done
k=0; for v in "$A" "$B"; do
  CANONSWAP_LIB=$v CANONSWAP_PROFILE_CSV=$O/layers_$k.csv timeout 600 python bench.py --full --no-cpu-baseline --no-fixed-job --no-chain --no-single-frame --steps 1 --warmup 2 > /dev/null 2>&1
  k=$((k+1))
done
python tools/cmp_layers.py $O/layers_0.csv $O/layers_1.csv 2>/dev/null | head -16 | tee $O/cmp.txt
