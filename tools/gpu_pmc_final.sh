#!/bin/bash
# The final tree's PMC passes of the headline bench (one rocprofv3 --pmc run per counter group,
# tools/profile_pmc.sh), their per-kernel summary, and the kernel stats of the same tree, so
# profiles/traffic_*.json can be regenerated from them (tools/traffic_json.py).
# Usage (GPU box): bash tools/gpu_pmc_final.sh <tag>     (results go to $SGN_OUT, default bench_out/)
set -eu
TAG=$1
OUT=${SGN_OUT:-bench_out}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $OUT
bash tools/profile_pmc.sh $OUT/pmc_$TAG > $OUT/pmc_$TAG.log 2>&1
python tools/pmc_summary.py $OUT/pmc_$TAG > $OUT/pmc_summary_$TAG.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/kst_$TAG -o run --output-format csv -- \
    python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extras > $OUT/kst_$TAG.json 2> $OUT/kst_$TAG.err
echo PMC_FINAL_DONE
