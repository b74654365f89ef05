"""The quasi-cyclic case of tests/test_gpu_rate_match.py, runnable in a process of its own
(python -m tests.rate_match_qc_child): the environment that picks the decoder's kernel
(LDPC_NO_QC_KERNEL) is read when a graph's device handle is made, so the table-kernel side needs a
fresh process.  Prints the counters of one batch as a JSON list."""
import json
import sys

from tests import codeword_util as cu

Z, SEED_BASE, B, P = 17, 5, 64, 0.03


def counters():
    import torch
    from iib_project_ldpc_codes_amd import qc
    from iib_project_ldpc_codes_amd.decoder import Quant
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    code = qc.random_base(3, 6, Z, SEED_BASE)
    rm = code.rate_match(punctured_cols=[0])
    mc = MonteCarlo(code.graph(), "bsc", P, cu.ITERS, algo="minsum", schedule="layered", quant=Quant(*cu.QUANT),
                    early_stop=True, seed=cu.SEED, batch=B, codewords="random", rate_match=rm)
    mc.run_batch(0, B)
    torch.cuda.synchronize()
    return [int(x) for x in mc.counters.cpu().numpy()]


if __name__ == "__main__":
    json.dump(counters(), sys.stdout)
