#!/bin/bash
# GPU-box check: parity tests, then a short bench, then (optionally) a rocprofv3 kernel trace.
# Stops at the first GPU fault / abort / timeout (exit codes other than pytest's 0/1).
# Logs go to $OUT (default build/gpu_check).
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-build/gpu_check}
mkdir -p $OUT
export TMPDIR=/tmp
STEPS=${STEPS:-10}
{ echo "nproc: $(nproc)"; echo "cpu.max: $(cat /sys/fs/cgroup/cpu.max 2>/dev/null)";
  python3 -c 'import os; print("affinity:", len(os.sched_getaffinity(0)))';
  grep -m1 "model name" /proc/cpuinfo; } > $OUT/hostinfo.txt 2>&1
timeout -k 10 ${TEST_TIMEOUT:-900} python -u -m pytest tests -m gpu -x -v --timeout ${PER_TEST_TIMEOUT:-300} --timeout-method thread ${PYTEST_ARGS:-} > $OUT/gpu_tests.log 2>&1
rc=$?
tail -30 $OUT/gpu_tests.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest exit $rc: stopping"; exit $rc; fi
if [ -n "$SKIP_BENCH" ]; then exit $rc; fi
timeout -k 10 ${BENCH_TIMEOUT:-600} python bench.py --full --steps $STEPS --warmup 2 ${BENCH_ARGS:-} > $OUT/bench.log 2>&1
brc=$?
tail -5 $OUT/bench.log
if [ $brc -ne 0 ]; then echo "bench exit $brc: stopping"; exit $brc; fi
if [ -n "$PROFILE" ]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run -- python bench.py --steps $STEPS --warmup 2 > $OUT/prof.log 2>&1
  echo "rocprof exit $?"
  find $OUT/prof -name "*stats*" | head
fi
exit $rc
