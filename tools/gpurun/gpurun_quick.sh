#!/bin/bash
# one GPU call: GPU tests (optionally a subset), per-launch network profile, bench without the CPU leg
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
TESTS=${TESTS:-tests}
timeout -k 10 400 python -u -m pytest $TESTS -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/tests.log 2>&1 || { tail -30 $OUT/tests.log; exit 1; }
tail -2 $OUT/tests.log
(timeout -k 10 200 python -u -m tools.profile_net > $OUT/profile_net.log 2>&1) || exit 1
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline > $OUT/bench.log 2>&1 || { tail -20 $OUT/bench.log; exit 1; }
tail -c 1500 $OUT/bench.log
