"""MonteCarlo(algo="gallager") sharded over a world-size-2 gloo group (CPU only), the pattern of
tests/test_multiprocess.py: the per-batch executor is tests/gallager_ref.py on the oracle's BSC words,
so this holds the trial partition, the per-round all-reduce and the global stop rule of a Gallager run
to one process's sequential counters -- independently of the kernels, which tests/test_gpu_gallager.py
holds to the same reference."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests import gallager_ref as ref
from tests import gallager_util as gu
from tests.test_multiprocess import _spawn

NAME, P, ITERS, B, FLIP, SEED = "r36_600", 0.03, 20, 32, 0, 11


def batch_counters(first_cw, Bn, remaining=0):
    """Counters of trials first_cw .. on the reference; remaining > 0: the sequential stop."""
    _, its, curve = ref.decode(gu.graph_csr(NAME), gu.bsc_bits(NAME, P, SEED, first_cw, Bn), ITERS, FLIP, True)
    return ref.mc_counters(curve, its, -1, remaining)


def _worker(rank, world, port, num_tests, stop_frames, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
        seen = []

        def executor(first_cw, Bn, stop, counters):  # the device executor's contract: the cut counts from counters[1]
            seen.append((first_cw, Bn, stop))
            rem = int(stop - counters[1]) if stop else 0
            if stop and rem <= 0:
                return
            counters += torch.from_numpy(batch_counters(first_cw, Bn, rem))

        mc = MonteCarlo(gu.graph(NAME), "bsc", P, ITERS, algo="gallager", flip_threshold=FLIP, seed=SEED, batch=B,
                        executor=executor)
        res = mc.run(num_tests=num_tests, stop_frame_errors=stop_frames)
        q.put((rank, seen, res["raw_counters"].tolist(), mc.rounds))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("num_tests,stop", [(5 * B + 7, 0), (0, 9)])
def test_sharded_gallager_run_matches_one_process(num_tests, stop):
    out = _spawn(_worker, 2, num_tests, stop)
    want = batch_counters(0, num_tests if num_tests else 16 * B, stop)
    assert want[0] == num_tests if num_tests else want[1] == stop
    for o in out:
        np.testing.assert_array_equal(np.array(o[2]), want)
    assert len({o[3] for o in out}) == 1
