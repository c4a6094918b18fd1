#!/bin/bash
# Runs on the GPU machine: bench + rocprofv3 kernel trace + three PMC passes (SQ, FETCH_SIZE, WRITE_SIZE -- separate passes, each on
# its own without any tracing: the counter file carries every dispatch's kernel name, grid and timestamps).  Every step has a time limit
# of its own and nothing runs behind a step that failed.  Outputs under $PROFILE_OUT (default profile_out/ in the repository); turn
# them into the tracked profiles/ files with `python scripts/summarize_profile.py TAG` afterwards (same PROFILE_OUT).
R=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-r02}
OUT=$R/${PROFILE_OUT:-profile_out}
export TMPDIR=/tmp
mkdir -p $OUT
cd /tmp
timeout -k 10 600 python3 $R/bench.py --full --steps 5 --warmup 1 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit $?
echo "bench done"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/bench_prof_$TAG.json 2> $OUT/prof_$TAG.err || exit $?
echo "kernel trace done"
timeout -k 10 400 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_LDS_BANK_CONFLICT --output-format csv -d $OUT/pmc_sq_$TAG -- python3 $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > $OUT/bench_sq_$TAG.json 2> $OUT/pmc_sq_$TAG.err || exit $?
echo "SQ counters done"
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_$TAG -- python3 $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > /dev/null 2> $OUT/pmc_fetch_$TAG.err || exit $?
echo "FETCH_SIZE done"
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write_$TAG -- python3 $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > /dev/null 2> $OUT/pmc_write_$TAG.err || exit $?
find $OUT -name "*.csv" -newer $OUT/bench_$TAG.json | head -20
cat $OUT/bench_$TAG.json
