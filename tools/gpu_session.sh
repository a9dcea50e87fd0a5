#!/bin/bash
# One measurement session on the current tree (run through gpurun from the
# repository root).  Usage: tools/gpu_session.sh TAG a|b
#   a  the whole GPU suite and smoke()
#   b  HBM traffic (FETCH / WRITE PMC passes) and VALU counters of C4 and C2,
#      the default bench line (C4, CPU baseline, records mode, the oracle's own
#      pipeline) reading them, rocprofv3 kernel statistics of the same
#      command, C2 and C3 bench lines
# Each step has its own time limit; the first failure ends the session.
# Results land in $OUT/ (copy what is judged to profiles/<round>/).
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
tag=$1
OUT=${ALVRL_OUT:-$R/results}   # where the logs and result lines go
export ALVRL_OUT=$OUT
cd "$R" && mkdir -p "$OUT"
export TMPDIR=/tmp
step() { echo "== $(date +%T) $*" >> "$OUT/steps_$tag.log"; }
if [ "$2" = a ]; then
  step suite && timeout -k 10 1100 python -u -m pytest tests -m gpu -v -s --timeout 300 --timeout-method thread \
      > "$OUT/pytest_$tag.log" 2>&1 \
  && step smoke && timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke_$tag.log" 2>&1 \
  && step done
else
  step pmc && "$R/tools/pmc_traffic.sh" C4 \
  && step pmcsum && python3 tools/pmc_summary.py C4 "$OUT" "$OUT/pmc_traffic_$tag.json" > /dev/null \
  && step valu4 && "$R/tools/pmc_valu.sh" C4 \
  && python3 tools/pmc_valu.py C4 "$OUT" $OUT/pmc_valu_C4.json tools/pairs_C4.json > /dev/null \
  && step valu2 && "$R/tools/pmc_valu.sh" C2 \
  && python3 tools/pmc_valu.py C2 "$OUT" $OUT/pmc_valu_C2.json tools/pairs_C2.json > /dev/null \
  && step bench && timeout -k 10 700 python bench.py --full --steps 10 --warmup 3 --pmc-json "$OUT/pmc_traffic_$tag.json" \
      --valu-json "$OUT/pmc_valu_{cfg}.json" > "$OUT/bench_$tag.json" 2> "$OUT/bench_$tag.err" \
  && step rocprof && (cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$tag" -o run \
      --output-format csv -- python3 "$R/bench.py" --no-cpu-baseline > "$OUT/prof_$tag.log" 2>&1) \
  && step c2 && timeout -k 10 300 python bench.py --config C2 --no-cpu-baseline --valu-json "$OUT/pmc_valu_{cfg}.json" \
      > "$OUT/bench_c2_$tag.json" 2> "$OUT/bench_c2_$tag.err" \
  && step c3 && timeout -k 10 300 python bench.py --config C3 --no-cpu-baseline > "$OUT/bench_c3_$tag.json" \
      2> "$OUT/bench_c3_$tag.err" \
  && step done
fi
rc=$?
echo "exit=$rc"
exit $rc
