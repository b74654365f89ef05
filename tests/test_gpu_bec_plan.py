"""Every BEC kernel instantiation a rate-1/2 graph can reach, run at the smallest call that
reaches it: each case first holds the call to the kernel its plan names (ldpc_debug_bec_plan,
tests/test_bec_plan.py holds the plan itself), then compares bit for bit with the oracle's
message_passing.c restatement.  (3,6) random_regular graphs, eps = 0.42, 20 iterations unless
said.  bec_dec_bits_kernel<512,4,u32> (no rate-1/2 graph plans to it) and
bec_mc_bits_kernel<512,2|4,u32> run on a graph of few checks (test_decode_wide_512, test_mc_wide_512).
"""
import functools

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


# The 512-thread rows that no rate-1/2 graph reaches need n > 4,096 with n + m small enough for four
# plane words within 72 KiB: 4,112 variables of degree 1 in 257 checks of degree 16 (the first multiple
# of 16 past 4,096).  Wider plane words are taken only from 1,024 workgroups on, so each case runs at
# the smallest B that selects its row (one codeword past 1,023 workgroups), not at one plane word plus
# one, and asserts that one codeword fewer selects the narrower row.
WIDE_N, WIDE_DC, WIDE_ITERS, WIDE_EPS = 4112, 16, 3, 0.1
WIDE_MC = [(65473, "bec_mc_bits_kernel<512,2,u32>", "bec_mc_bits_kernel<512,1,u32>"),
           (130945, "bec_mc_bits_kernel<512,4,u32>", "bec_mc_bits_kernel<512,2,u32>")]


def _wide_graph():
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    if "wide" not in _graphs:
        _graphs["wide"] = TannerGraph.random_regular(WIDE_N, 1, WIDE_DC, seed=11)
    return _graphs["wide"]


def _wide_name(mode, B):
    return bec_plans(WIDE_N, WIDE_N // WIDE_DC, [(mode, B, WIDE_ITERS)], dc=WIDE_DC)[0]["name"]


def test_decode_wide_512(torch):
    """bec_dec_bits_kernel<512,4,u32>: as test_decode, 65,473 words of 64 distinct ones."""
    from iib_project_ldpc_codes_amd import decoder
    n, B, iters = WIDE_N, 65473, WIDE_ITERS
    assert _wide_name(BEC_DECODE, B) == "bec_dec_bits_kernel<512,4,u32>"
    assert _wide_name(BEC_DECODE, B - 1) == "bec_dec_bits_kernel<512,2,u32>"
    g = _wide_graph()
    words, errin = _perturbed_bec_batch(n, DISTINCT, WIDE_EPS, iters, seed=n + B)
    ow, oerr, oits = oracle.bec_decode_batch(words, iters, g.variable_lookup, g.check_lookup, n, g.k, 1, WIDE_DC,
                                             errors=errin)
    assert 0 < np.count_nonzero(ow == 2) < np.count_nonzero(words == 2)  # some erasures decode, some stay
    row = np.arange(B) % len(words)
    w, err, its = decoder.bec_decode(g, words[row], iters, errors=errin[row])
    np.testing.assert_array_equal(w.astype(np.int8), ow[row])
    np.testing.assert_array_equal(err, oerr[row])
    np.testing.assert_array_equal(its, oits[row])


@functools.lru_cache(maxsize=None)
def _wide_mc_reference():
    """Per-trial error curves and iteration counts of trials 0 .. 130,944 (the oracle's channel and
    decoder, once for both cases: trial b does not depend on the batch it is drawn in)."""
    g, B = _wide_graph(), max(b for b, _, _ in WIDE_MC)
    words = oracle.channel(oracle.CH_BEC, WIDE_EPS, 9, 0, WIDE_N, B)
    erased = np.count_nonzero(words == 2, axis=1)
    _, err, its = oracle.bec_decode_batch(words, WIDE_ITERS, g.variable_lookup, g.check_lookup, WIDE_N, g.k, 1, WIDE_DC)
    curves = np.concatenate([erased[:, None], err], axis=1)
    for a in (curves, its):
        a.setflags(write=False)
    return curves, its


@pytest.mark.parametrize("B,name,narrower", WIDE_MC)
def test_mc_wide_512(torch, B, name, narrower):
    """bec_mc_bits_kernel<512,2,u32> and <512,4,u32>: every counter and the curve, as test_mc."""
    assert _wide_name(BEC_MC, B) == name and _wide_name(BEC_MC, B - 1) == narrower
    got = _mc_counters(_wide_graph(), "bec", WIDE_EPS, 9, B, WIDE_ITERS)
    curves, its = (a[:B] for a in _wide_mc_reference())
    assert 0 < curves[:, -1].sum() < curves[:, 0].sum()  # some erasures decode, some stay
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
