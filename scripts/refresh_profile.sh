#!/bin/bash
# Build container: regenerate profiles/<TAG>_* and profiles/counters.json for the CURRENT kernel sources (two gpurun calls: the profiled
# passes, then -- with the fresh counters in place -- the bench line that carries them).  Usage: GPU_RUN=<runner> bash scripts/refresh_profile.sh r03i
# (GPU_RUN: the command that runs its one argument, a shell command, in a copy of this tree on an MI355X and copies $PROFILE_OUT back)
set -e
TAG=${1:?tag}
RUN=${GPU_RUN:?set GPU_RUN to the command that runs a shell command on an MI355X}
OUT=${PROFILE_OUT:-profile_out}
cd "$(dirname "$0")/.."
python -c "import __graft_entry__ as g; g.build()"
$RUN "mkdir -p $OUT && PROFILE_OUT=$OUT bash scripts/profile_bench.sh $TAG > $OUT/profile_$TAG.log 2>&1; tail -c 300 $OUT/profile_$TAG.log"
PROFILE_OUT=$OUT python scripts/summarize_profile.py $TAG | tail -3
$RUN "mkdir -p $OUT && python bench.py --full --steps 5 --warmup 1 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err; tail -c 200 $OUT/bench_$TAG.json"
cp $OUT/bench_$TAG.json profiles/${TAG}_bench.json
python - <<PY
import json
d = json.load(open("profiles/${TAG}_bench.json"))
r = d["roofline"]
print("ms_per_step %.2f  frac %s  issue-slot frac %s  bound-pass MFMA frac %.3f  counters: %s" % (d["ms_per_step"], r["frac"], r["issue_slots"]["frac"], r["bound_pass"]["frac"], r["counters"]))
PY
