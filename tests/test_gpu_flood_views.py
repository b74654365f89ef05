"""The two views of the flooding loop (csrc/bp_flood.hpp) agree with each other: the same frames
decoded by bp_generic_kernel (CSR view, decoder.bp_decode on the TannerGraph of fallback_csr) and
by bp_ens_kernel (ensemble view, decoder.bp_ensemble_decode_dev on the graph's two lists repeated
for every word) give bit-identical post / hard / its, sum-product included.

The graphs are tests.graph_util.regular_simple(n, dv, dc, seed=1), the smallest that reach every
check width and both storage modes:
  r58_320    <8,lds>    dv = 5: the looped variable path of both views
  r510_640   <16,lds>
  r432_2048  <32,lds>   dv = 4: the register path
  r510_9000  <16,gmem>  messages really in the slab on both sides
The edge order is the same on both sides: csr_from_checks gives each variable's slots ascending,
and on a regular graph (slot = c dc + j) ascending slots are ascending checks, variable_lookup's
order -- so the variable sums add in the same order.  Each case first holds both calls to the
kernels named here (the plans), and the generic min-sum result to the oracle, so the pair cannot
agree on a wrong answer.
"""
import numpy as np
import pytest

from oracle import oracle
from tests.graph_util import FALLBACK_KERNELS, bp_plans, fallback_csr, fallback_regular
from tests.test_ens_plan import ens_plans
from tests.test_gpu_fallback import UNSAT_SIGMA

pytestmark = pytest.mark.gpu

B = 4
ALPHA = 0.75
ENS_KERNEL = {"r58_320": "bp_ens_kernel<8,lds>", "r510_640": "bp_ens_kernel<16,lds>",
              "r432_2048": "bp_ens_kernel<32,lds>", "r510_9000": "bp_ens_kernel<16,gmem>"}
MODES = [(False, 3), (True, 20)]  # (early stop, iterations)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


@pytest.mark.parametrize("name", list(ENS_KERNEL))
def test_views_bit_identical(torch, name):
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    csr = fallback_csr(name)
    g = TannerGraph.from_csr(*csr)
    lists = fallback_regular(name)
    n, dv, dc = lists.n, lists.dv, lists.dc
    chk = np.asarray(lists.check_lookup, np.int32)
    var = np.asarray(lists.variable_lookup, np.int32)
    assert np.all(np.diff(var.reshape(n, dv), axis=1) > 0)  # each variable's checks ascending
    np.testing.assert_array_equal(chk, csr[1])  # the same graph, slot for slot
    # both calls run the kernels named here, the gmem pair with messages really in the slab
    calls = [(algo, int(es), 0, 1, iters, B) for algo in (0, 1) for es, iters in MODES]
    rc, eplans = ens_plans(n, dv, dc, calls)
    assert rc == 0
    for call, p, ep in zip(calls, bp_plans(csr, calls), eplans):
        assert p["name"] == FALLBACK_KERNELS[name] and ep["name"] == ENS_KERNEL[name], (name, call, p, ep)
        assert FALLBACK_KERNELS[name].split("<")[1] == ENS_KERNEL[name].split("<")[1]  # same width and storage
        if "gmem" in p["name"]:
            assert 0 < p["lds_slots"] < n * dv and 0 < ep["lds_slots"] < n * dv, (name, call, p, ep)
    for early_stop in (False, True):
        assert g.kernel_name(early_stop=early_stop) == FALLBACK_KERNELS[name]
    llr = oracle.channel(oracle.CH_AWGN, UNSAT_SIGMA[name], 13, 0, n, B)
    d_llr = torch.from_numpy(np.array(llr)).cuda()
    d_chk = torch.from_numpy(np.tile(chk, (B, 1))).cuda()
    d_var = torch.from_numpy(np.tile(var, (B, 1))).cuda()
    for algo, alpha in (("minsum", ALPHA), ("spa", 1.0)):
        for early_stop, iters in MODES:
            post, hard, its = decoder.bp_decode(g, llr, iters, algo, alpha, early_stop)
            if algo == "minsum":
                opost, ohard, oits = oracle.bp_decode_batch(csr, llr, iters, 1, ALPHA, early_stop)
                np.testing.assert_array_equal(post, opost)
                np.testing.assert_array_equal(hard, ohard)
                np.testing.assert_array_equal(its, oits)
            epost, ehard, eits = decoder.bp_ensemble_decode_dev(n, dv, dc, d_chk, d_var, d_llr, iters, algo, alpha,
                                                                early_stop)
            torch.cuda.synchronize()
            assert np.array_equal(epost.cpu().numpy().view(np.uint32), np.asarray(post).view(np.uint32)), (algo, iters)
            np.testing.assert_array_equal(ehard.cpu().numpy(), hard)
            np.testing.assert_array_equal(eits.cpu().numpy(), its)
