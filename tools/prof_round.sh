#!/bin/bash
# One GPU call: kernel-trace stats + PMC passes of bench.py, the SG bench and a kernel trace of
# the training bench.  Usage (GPU box): bash tools/prof_round.sh <tag>
# Results go to $SGN_OUT (default bench_out/).
set -u
TAG=$1; shift
OUT=${SGN_OUT:-bench_out}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- \
    python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $OUT/prof_$TAG.json 2> $OUT/prof_$TAG.err || { echo PROF_FAIL; tail $OUT/prof_$TAG.err; exit 1; }
cat $OUT/prof_$TAG.json
timeout -k 10 300 python bench.py --full --no-cpu-baseline --sg > $OUT/benchsg_$TAG.json 2> $OUT/benchsg_$TAG.err || { echo SG_FAIL; tail $OUT/benchsg_$TAG.err; exit 1; }
cat $OUT/benchsg_$TAG.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/proftrain_$TAG -o run --output-format csv -- \
    python bench.py --train > $OUT/proftrain_$TAG.json 2> $OUT/proftrain_$TAG.err || { echo TRAINPROF_FAIL; tail $OUT/proftrain_$TAG.err; exit 1; }
cat $OUT/proftrain_$TAG.json
KREGEX="k_agg_rows|k_knn|k_march|k_color|k_composite" timeout -k 10 900 bash tools/profile_pmc.sh $OUT/pmc_$TAG \
    > $OUT/pmc_$TAG.out 2>&1 || { echo PMC_FAIL; tail $OUT/pmc_$TAG.out; exit 1; }
echo PROF_ROUND_DONE
