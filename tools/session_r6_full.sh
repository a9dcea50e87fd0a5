#!/bin/bash
# Round-6 session: the GPU suite (plugin run and C5 first), smoke and a default bench on the current tree
set -o pipefail
T=${1:-r6b}
OUT=${ALVRL_OUT:-results}   # where the logs and result lines go
mkdir -p "$OUT"
timeout -k 10 900 python3 -u -m pytest tests/test_gpu_plugin_run.py tests/test_gpu_scale.py -x -q -s --timeout 600 --timeout-method thread > $OUT/pytest_first_$T.log 2>&1 &&
timeout -k 10 1100 python3 -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread --deselect tests/test_gpu_scale.py::test_c5_end_to_end > $OUT/pytest_$T.log 2>&1 &&
timeout -k 10 120 python3 -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$T.log 2>&1 &&
timeout -k 10 400 python3 -u bench.py --full > $OUT/bench_$T.json 2> $OUT/bench_$T.err
