#!/bin/bash
# GPU box: alternating bench runs under two environment settings on the same box, then per-layer CSVs of both -> out/<tag>/:
#   bash tools/ab_env.sh CANONSWAP_HALO_PERSIST=0 CANONSWAP_HALO_PERSIST=1 [rounds] [tag]
A=$1; B=$2; R=${3:-2}; TAG=${4:-ab_env}
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; O=$ROOT/out/$TAG; mkdir -p $O
for i in $(seq $R); do for v in "$A" "$B"; do
  env $v timeout 600 python bench.py --full --steps 10 --warmup 3 --no-fixed-job --no-cpu-baseline > $O/b.json 2>$O/b.err
  python - <<PY | tee -a $O/ab.txt
import json
try:
    d=json.loads(open("$O/b.json").read().strip().splitlines()[-1]); print("env=[$v]", d["value"], d["roofline"]["frac"], d["ms_per_step"], d.get("psnr_db_min"))
except Exception as e: print("env=[$v] failed", e, open("$O/b.err").read()[-1500:])
PY
done; done
k=0; for v in "$A" "$B"; do
  env $v CANONSWAP_PROFILE_CSV=$O/layers_$k.csv timeout 600 python bench.py --full --no-cpu-baseline --no-fixed-job --steps 1 --warmup 2 > /dev/null 2>&1
  k=$((k+1))
done
python tools/cmp_layers.py $O/layers_0.csv $O/layers_1.csv 2>/dev/null | head -24 | tee $O/cmp.txt
