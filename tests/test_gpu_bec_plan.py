"""Every BEC kernel instantiation a rate-1/2 graph can reach, run at the smallest call that
reaches it: each case first holds the call to the kernel its plan names (ldpc_debug_bec_plan,
tests/test_bec_plan.py holds the plan itself), then compares bit for bit with the oracle's
message_passing.c restatement.  (3,6) random_regular graphs, eps = 0.42, 20 iterations unless
said.  Without a GPU run, as before: bec_dec_bits_kernel<512,4,u32> (no rate-1/2 graph plans to
it) and bec_mc_bits_kernel<512,2|4,u32>.
"""
import numpy as np
import pytest

from oracle import oracle
from tests.graph_util import BEC_DECODE, BEC_ENS_MC, BEC_MC, bec_plans
from tests.test_gpu_parity import _mc_counters, _perturbed_bec_batch
from tests.test_gpu_peel import _oracle_trials, _peel_stats, _per_trial

pytestmark = pytest.mark.gpu

EPS = 0.42


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


_graphs = {}


def _graph(n):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    if n not in _graphs:
        _graphs[n] = TannerGraph.random_regular(n, 3, 6, seed=11)
    return _graphs[n]


def _name(mode, n, B, iters):
    return bec_plans(n, n // 2, [(mode, B, iters)])[0]["name"]


# Above 64 distinct words the batch repeats them: the oracle decodes 64, every tile must equal it
DISTINCT = 64


@pytest.mark.parametrize("n,B,iters,name", [
    (96, 3, 20, "bec_kernel<256>"),
    (4096, 3, 20, "bec_kernel<1024>"),
    (96, 70, 20, "bec_dec_bits_kernel<256,1,u32>"),       # partial last workgroup
    (4098, 70, 20, "bec_dec_bits_kernel<512,1,u32>"),
    (26700, 66, 20, "bec_dec_bits_kernel<1024,1,u8>"),
    (107000, 66, 50, "bec_kernel<1024>"),                 # planes of no width fit: B >= 64 on bec_kernel
    (96, 32737, 20, "bec_dec_bits_kernel<256,2,u32>"),
    (96, 65473, 20, "bec_dec_bits_kernel<256,4,u32>"),
    (4098, 32737, 20, "bec_dec_bits_kernel<512,2,u32>"),
])
def test_decode(torch, n, B, iters, name):
    from iib_project_ldpc_codes_amd import decoder
    assert _name(BEC_DECODE, n, B, iters) == name
    g = _graph(n)
    words, errin = _perturbed_bec_batch(n, min(B, DISTINCT), EPS, iters, seed=n + B)
    ow, oerr, oits = oracle.bec_decode_batch(words, iters, g.variable_lookup, g.check_lookup, n, n // 2, 3, 6,
                                             errors=errin)
    row = np.arange(B) % len(words)
    w, err, its = decoder.bec_decode(g, words[row], iters, errors=errin[row])
    np.testing.assert_array_equal(w.astype(np.int8), ow[row])
    np.testing.assert_array_equal(err, oerr[row])
    np.testing.assert_array_equal(its, oits[row])


@pytest.mark.parametrize("n,B,iters,name", [
    (96, 40, 20, "bec_mc_bits_kernel<256,1,u32>"),
    (96, 65473, 20, "bec_mc_bits_kernel<256,2,u32>"),
    (96, 131072, 20, "bec_mc_bits_kernel<256,4,u32>"),
    (4098, 40, 20, "bec_mc_bits_kernel<512,1,u32>"),
    (26600, 10, 20, "bec_mc_bits_kernel<1024,1,u8>"),
    (107000, 3, 50, "bec_kernel<1024>"),
])
def test_mc(torch, n, B, iters, name):
    assert _name(BEC_MC, n, B, iters) == name
    g = _graph(n)
    got = _mc_counters(g, "bec", EPS, 9, B, iters)
    words = oracle.channel(oracle.CH_BEC, EPS, 9, 0, n, B)
    _, err, its = oracle.bec_decode_batch(words, iters, g.variable_lookup, g.check_lookup, n, n // 2, 3, 6)
    curves = np.concatenate([np.count_nonzero(words == 2, axis=1)[:, None], err], axis=1)
    want = np.concatenate([[B, np.count_nonzero(curves[:, -1]), curves[:, -1].sum(), its.sum()], curves.sum(axis=0)])
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("n,B,iters,name", [
    (96, 40, 20, "bec_peel_kernel<1024>"),
    (80000, 2, 20, "bec_kernel<1024>"),  # the check state does not fit LDS: the fallback
])
def test_ensemble_mc(torch, n, B, iters, name):
    """Trial by trial (curves and iteration counts), then the B trials as one batch; the
    peeling decoder counts the trials it decodes."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    assert {_name(BEC_ENS_MC, n, b, iters) for b in (1, B)} == {name}
    before = _peel_stats()[2]
    got_c, got_i = _per_trial(torch, n, EPS, iters, 31, B)
    want_c, want_i = _oracle_trials(n, EPS, iters, 31, B)
    np.testing.assert_array_equal(got_c, want_c)
    np.testing.assert_array_equal(got_i, want_i)
    mc = MonteCarlo.ensemble(n, 3, 6, "bec", EPS, iters, seed=31, batch=B, expurgation=-1)
    mc.run_batch(0, B)
    torch.cuda.synchronize()
    c = mc.counters.cpu().numpy()
    assert c[0] == B and c[3] == want_i.sum()
    np.testing.assert_array_equal(c[4:], want_c.sum(axis=0))
    assert _peel_stats()[2] - before == (2 * B if "peel" in name else 0)
