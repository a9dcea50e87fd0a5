#!/bin/bash
# The other BASELINE configurations on the current tree: C2 (brute force,
# 10k VRLs) and C3 (fixed-depth LightSlice), plus C2's rocprofv3 kernel
# statistics.  Each GPU step has its own limit; the first failure ends it.
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
T=${1:-cfg}
OUT=${ALVRL_OUT:-$R/results}   # where the logs and result lines go
cd "$R" && mkdir -p "$OUT"
export TMPDIR=/tmp
step() { echo "== $(date +%T) $*" >> $OUT/steps_$T.log; }
step c2 && timeout -k 10 400 python bench.py --full --config C2 > $OUT/bench_c2_$T.json 2> $OUT/bench_c2_$T.err \
 && step c3 && timeout -k 10 400 python bench.py --full --config C3 > $OUT/bench_c3_$T.json 2> $OUT/bench_c3_$T.err \
 && step rocprof_c2 && (cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof_c2_$T" -o run --output-format csv -- python3 "$R/bench.py" --config C2 --no-cpu-baseline > "$OUT/prof_c2_$T.log" 2>&1) \
 && step done
echo "exit=$?"
