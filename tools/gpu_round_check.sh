#!/bin/bash
# gpu_round_check.sh <tag>: round-end check of the committed tree: GPU suite, smoke, full bench (window + solve sets + CPU baseline),
# the multi-rank bench path at world 1 (RCCL stats exchange), each step under its own limit.
# Logs go to $OUT/<tag> (default build/round_check/<tag>).
cd "$(dirname "$0")/.." || exit 1
t=${1:-r2}
OUT=${OUT:-build/round_check}/$t
mkdir -p $OUT
export TMPDIR=/tmp
set -o pipefail
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { tail -30 $OUT/gpu_tests.log; exit 1; }
tail -1 $OUT/gpu_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 1; }
timeout -k 10 600 python bench.py --full > $OUT/bench.log 2>&1 || { tail -20 $OUT/bench.log; exit 1; }
TOG_BENCH_DIST=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29513 RANK=0 WORLD_SIZE=1 LOCAL_RANK=0 timeout -k 10 600 python bench.py --full --no-cpu-baseline > $OUT/bench_dist1.log 2>&1 || { tail -20 $OUT/bench_dist1.log; exit 1; }
tail -c 1200 $OUT/bench.log
