#!/bin/bash
# GPU box: parity tests, then the full bench (extras + CPU baselines; BENCH_ARGS overrides).
# Stops at the first crash / timeout.  Logs go to $LOG_DIR (default bench_logs/).
set -u
LOG_DIR=${LOG_DIR:-bench_logs}
mkdir -p $LOG_DIR
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 ${TEST_TIMEOUT:-900} python -m pytest tests -m gpu -q ${PYTEST_ARGS:--x} > $LOG_DIR/gpu_tests.log 2>&1
rc=$?
echo "pytest rc=$rc"; tail -30 $LOG_DIR/gpu_tests.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
if [ "${RUN_BENCH:-1}" = "1" ]; then
  timeout -k 10 ${BENCH_TIMEOUT:-400} python bench.py ${BENCH_ARGS:---full} > $LOG_DIR/bench.log 2>&1
  brc=$?
  echo "bench rc=$brc"; tail -5 $LOG_DIR/bench.log
  exit $brc
fi
exit $rc
