#!/bin/bash
# one GPU call: GPU tests, smoke, full bench (+CPU baseline), rocprof kernel stats of a short bench
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/tests.log 2>&1 || { tail -30 $OUT/tests.log; exit 1; }
tail -2 $OUT/tests.log
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
timeout -k 10 600 python -u bench.py --full > $OUT/bench.log 2>&1 || { tail -20 $OUT/bench.log; exit 1; }
tail -c 3000 $OUT/bench.log
[ -n "$NO_PROF" ] && exit 0
bash tools/gpurun/gpurun_prof.sh
