#!/bin/bash
# Round-end evidence: full GPU suite, default bench (window + whole-solve leg + CPU baseline), profile of the
# bench window (trace, FETCH/WRITE, SQ), Kuka trace, tail bench. Each GPU step under its own limit.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-build/final}
mkdir -p $OUT
export TMPDIR=/tmp
set -o pipefail
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { tail -30 $OUT/gpu_tests.log; exit 1; }
tail -1 $OUT/gpu_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 1; }
timeout -k 10 600 python bench.py --full > $OUT/bench.log 2>&1 || { tail -20 $OUT/bench.log; exit 1; }
TAG=r2c bash tools/profile_round.sh > $OUT/pr_r2c.log 2>&1 || exit 1
TAG=r2ckuka STEPS=10 NO_SQ=1 BENCH_ARGS="--workload kuka" bash tools/profile_round.sh > $OUT/pr_r2ckuka.log 2>&1 || exit 1
for w in cartpole quad_maze maze_infeasible; do
  timeout -k 10 300 python bench.py --workload $w --steps 10 --warmup 2 --no-cpu-baseline --no-solve-leg > $OUT/bench_$w.log 2>&1 || exit 1
done
timeout -k 10 300 python bench.py --batch 1 --steps 10 --warmup 2 --no-cpu-baseline --no-solve-leg > $OUT/tail_b1.log 2>&1 || exit 1
tail -c 800 $OUT/bench.log
