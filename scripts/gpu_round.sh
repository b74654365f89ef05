#!/bin/bash
# GPU box: the round-end sequence -- parity tests, smoke(), the full bench line (extras + CPU
# baselines), and the distributed code path of bench.py under torchrun (1 rank, RCCL).
# Logs go to $LOG_DIR (default bench_logs/).
set -u
LOG_DIR=${LOG_DIR:-bench_logs}
mkdir -p $LOG_DIR
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $LOG_DIR/gpu_tests.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -3 $LOG_DIR/gpu_tests.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $LOG_DIR/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -2 $LOG_DIR/smoke.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python bench.py --full > $LOG_DIR/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; grep metric $LOG_DIR/bench.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --steps 3 --warmup 1 > $LOG_DIR/bench_dist.log 2>&1
rc=$?; echo "bench torchrun rc=$rc"; grep metric $LOG_DIR/bench_dist.log | cut -c1-300
exit $rc
