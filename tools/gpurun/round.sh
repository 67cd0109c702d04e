#!/bin/bash
# one GPU call: GPU tests, smoke, default bench (all legs); logs under $OUT/
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
TESTS=${TESTS:-tests}
timeout -k 10 900 python -u -m pytest $TESTS -m gpu -v --timeout 400 --timeout-method thread > $OUT/tests.log 2>&1 || { tail -40 $OUT/tests.log; exit 1; }
tail -3 $OUT/tests.log
[ -n "$NO_BENCH" ] && exit 0
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
timeout -k 10 600 python -u bench.py --full ${BENCH_ARGS} > $OUT/bench.log 2>&1 || { tail -30 $OUT/bench.log; exit 1; }
tail -c 4000 $OUT/bench.log
