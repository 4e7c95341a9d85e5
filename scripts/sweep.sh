#!/bin/bash
# A/B sweep of launch/feature knobs at the bench config (one bench process per point; the env knobs
# are read at context creation). Usage (GPU box, repo root): scripts/sweep.sh <tag> "<ENV=.. ENV=..>" ...
# Results go to $SF_OUT_DIR/<tag>/ (default bench_out/<tag>/).
set -e
TAG=$1; shift
OUT=${SF_OUT_DIR:-bench_out}/$TAG
mkdir -p $OUT
i=0
for cfg in "$@"; do
  i=$((i+1))
  env $cfg timeout -k 10 120 python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline > $OUT/p$i.json 2> $OUT/p$i.err
  echo "$cfg => $(python3 -c "import json;d=json.loads(open('$OUT/p$i.json').readlines()[-1]);print(d['value'],d['ms_per_step'])")"
done
