#!/bin/bash
# one GPU call: bench (+cpu baseline), rocprofv3 kernel stats, per-launch profile
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
timeout -k 10 400 python -u bench.py --full > $OUT/bench.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run -- python3 bench.py --full --steps 20 --warmup 3 --no-cpu-baseline > $OUT/bench_prof.log 2>&1 || exit $?
timeout -k 10 200 python -u -m tools.profile_net > $OUT/profile_net.log 2>&1
