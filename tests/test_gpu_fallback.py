"""The soft decoders' fallback kernels -- bp_irr_kernel with DC = 8 and bp_generic_kernel<8|16|32,
lds|gmem>, which serve every graph without a local-edge or (3,6) lane layout -- against the
oracle, at check degrees 7-32 (tests/graph_util.FALLBACK_KERNELS: regular (4,8), (5,8), (5,10),
(3,24), (4,32) graphs at a size that keeps every message in LDS and at one that puts messages
into the per-workgroup slab, and two graphs of mixed check degrees).

Every test first holds the launch plan of its own calls (bp_plans) and the device graph
(kernel_name) to the kernel the table names, so a change of the plan cannot move a case to
another kernel unnoticed; the gmem cases also need 0 < lds_slots < E (messages really stored in
the slab).

* Min-sum: post / hard / its bit-exact with the oracle, fixed count and early stop, 1 / 3 / 20
  iterations, on BI-AWGN frames and on the fp32 edge values of graph_util.extreme_llrs.
* Sum-product, unsaturated (a sigma per graph at which the oracle's posteriors stay below the
  23 ln 2 message clamp, asserted): 1 / 3 / 5 iterations within SPA_ATOL + SPA_RTOL |post|, the
  project's 1e-4 / 1e-4.  The CPU restatement of the kernels' rescaled check rule (oracle algo
  3) is within 2.9e-6 of the double rule on these frames, so the hardware's 1-ulp v_exp / v_log /
  v_rcp leave a wide margin.
* Sum-product, saturated (high SNR: every message at the clamp within a few iterations), 3 and
  10 iterations, fixed count and early stop: finite posteriors within SAT_ATOL + SAT_RTOL |post|
  (tests/test_gpu_edges.py's saturated tolerance), decisions differing only where the oracle's
  posterior is within SAT_ATOL of 0, early-stop iteration counts equal on >= 98 % of frames.
  Before check_update<0, D > 6> rescaled its (E, O) sums, six saturated inputs overflowed fp32
  (2^138) and these posteriors were NaN -- read as hard decision 0, i.e. "decoded".
* More codewords than workgroups (B = 264 > the 256-workgroup grid of the slab kernels): the
  b += gridDim.x loop and the reuse of a slab by a second codeword.
* Fused Monte-Carlo: min-sum on BSC, every counter and the whole per-iteration curve bit-exact;
  sum-product on BI-AWGN within tests/test_gpu_loc.py::test_loc_mc_spa_vs_oracle's tolerances,
  at a sigma where the oracle alone has both decoded and failed frames.

The two small bp_irr_kernel graphs ((4,8) n = 256 and mixA: 1 and 2 variables per thread) had a
plan but no kernel instantiation before this module existed; every call on them was refused.

Each sum-product case dumps its achieved margins (tests/test_gpu_fullsize.py's _dump).
"""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests.graph_util import FALLBACK_KERNELS, bp_plans, extreme_llrs, fallback_csr
from tests.test_gpu_fullsize import _dump

pytestmark = pytest.mark.gpu

SPA_ATOL, SPA_RTOL = 1e-4, 1e-4   # tests/test_gpu_parity.py
SAT_ATOL, SAT_RTOL = 1e-3, 3e-3   # tests/test_gpu_edges.py
XMAX = 23 * np.log(2.0)           # the message clamp (oracle ORACLE_XMAX)
B = 24

# sigma per graph at which max |oracle posterior| < XMAX after 1, 3 and 5 iterations of the
# test's frames (the smallest multiple of 0.05 that leaves a 5 % margin, found on the CPU)
UNSAT_SIGMA = {"r48_256": 0.90, "r48_9216": 0.90, "r58_320": 0.95, "r58_8800": 1.00, "r510_640": 0.85,
               "r510_9000": 0.85, "r324_1024": 0.75, "r432_2048": 0.80, "r432_12288": 0.80, "mixA": 1.25,
               "mixB": 1.00}
# graph, sigma: the oracle's posteriors exceed the clamp from the first iterations on
SATURATED = [("r48_256", 0.75), ("r48_256", 0.6), ("r510_640", 0.6), ("r324_1024", 0.35), ("r432_2048", 0.3)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


@functools.lru_cache(maxsize=None)
def _case(name):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    csr = fallback_csr(name)
    return TannerGraph.from_csr(*csr), csr


def _routed(name, calls, early_stop=None):
    """The plans of `calls` (algo, early_stop, mc, want_post, iters, B) on graph `name`, each held
    to the kernel FALLBACK_KERNELS names; early_stop: also ask the device graph itself."""
    g, csr = _case(name)
    want = FALLBACK_KERNELS[name]
    plans = bp_plans(csr, calls)
    for call, p in zip(calls, plans):
        assert p["name"] == want, (name, call, p)
        if "gmem" in want:
            assert 0 < p["lds_slots"] < csr[1].size, (name, call, p)
    if early_stop is not None:
        assert g.kernel_name(early_stop=early_stop) == want
    return plans


def _decode(g, llr, iters, algo, alpha=1.0, early_stop=False):
    from iib_project_ldpc_codes_amd import decoder
    return decoder.bp_decode(g, llr, iters, algo, alpha, early_stop)


def _mc_counters(g, channel, p, seed, batch, iters, algo, alpha, early_stop):
    import torch
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    mc = MonteCarlo(g, channel, p, iters, algo=algo, alpha=alpha, early_stop=early_stop, seed=seed, batch=batch)
    mc.run_batch(0, batch)
    torch.cuda.synchronize()
    return mc.counters.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _awgn(n, sigma, seed, frames):
    return oracle.channel(oracle.CH_AWGN, sigma, seed, 0, n, frames)


def _spa_margins(post, opost):
    d = np.abs(post.astype(np.float64) - opost)
    ref = np.abs(opost.astype(np.float64))
    return {"post_max_abs": float(np.nanmax(d)) if np.isfinite(d).any() else None,
            "oracle_post_max_abs": float(ref.max()),
            "within_spa_tol_frac": float((d <= SPA_ATOL + SPA_RTOL * ref).mean()),
            "nan_count": int(np.isnan(post).sum())}


# ------------------------------------------------------------------ min-sum
@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("name", list(FALLBACK_KERNELS))
def test_minsum_bit_exact(torch, name, early_stop):
    g, csr = _case(name)
    _routed(name, [(1, int(early_stop), 0, 1, it, B) for it in (1, 3, 20)], early_stop)
    for llr in (_awgn(g.n, 0.80, 13, B), extreme_llrs(g.n, B, 11)):
        for iters in (1, 3, 20):
            post, hard, its = _decode(g, llr, iters, "minsum", 0.75, early_stop)
            opost, ohard, oits = oracle.bp_decode_batch(csr, llr, iters, 1, 0.75, early_stop)
            np.testing.assert_array_equal(hard, ohard)
            np.testing.assert_array_equal(its, oits)
            np.testing.assert_array_equal(post, opost)


# -------------------------------------------------------------- sum-product
@pytest.mark.parametrize("name", list(FALLBACK_KERNELS))
def test_spa_unsaturated_posterior_tolerance(torch, name):
    g, csr = _case(name)
    _routed(name, [(0, 0, 0, 1, it, B) for it in (1, 3, 5)], False)
    sigma = UNSAT_SIGMA[name]
    llr = _awgn(g.n, sigma, 21, B)
    stats = {"graph": name, "kernel": FALLBACK_KERNELS[name], "sigma": sigma}
    got = {}
    for iters in (1, 3, 5):
        post, hard, its = _decode(g, llr, iters, "spa")
        opost, ohard, _ = oracle.bp_decode_batch(csr, llr, iters, 0)
        assert np.abs(opost).max() < XMAX  # the case is what it claims: nothing at the clamp
        stats["iters%d" % iters] = _spa_margins(post, opost)
        got[iters] = (post, opost, its)
    _dump("fallback_spa_unsat_" + name, stats)
    for iters, (post, opost, its) in got.items():
        np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL, err_msg=str(stats))
        assert np.all(its == iters)


@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("name,sigma", SATURATED)
def test_spa_saturated(torch, name, sigma, early_stop):
    g, csr = _case(name)
    _routed(name, [(0, int(early_stop), 0, 1, it, 32) for it in (3, 10)], early_stop)
    llr = _awgn(g.n, sigma, 3, 32)
    stats = {"graph": name, "kernel": FALLBACK_KERNELS[name], "sigma": sigma, "early_stop": early_stop}
    got = {}
    for iters in (3, 10):
        post, hard, its = _decode(g, llr, iters, "spa", 1.0, early_stop)
        opost, ohard, oits = oracle.bp_decode_batch(csr, llr, iters, 0, 1.0, early_stop)
        s = _spa_margins(post, opost)
        s["its_equal_frac"] = float(np.mean(its == oits))
        s["oracle_fer"] = float(ohard.any(axis=1).mean())
        stats["iters%d" % iters] = s
        got[iters] = (post, hard, its, opost, ohard, oits)
    _dump("fallback_spa_sat_%s_sigma%.2f_%s" % (name, sigma, "es" if early_stop else "fixed"), stats)
    assert max(stats["iters%d" % it]["oracle_post_max_abs"] for it in (3, 10)) > XMAX, stats  # saturated indeed
    for iters, (post, hard, its, opost, ohard, oits) in got.items():
        assert np.isfinite(post).all(), stats
        d = np.abs(post.astype(np.float64) - opost)
        assert np.all(d <= SAT_ATOL + SAT_RTOL * np.abs(opost)), stats
        diff = hard != ohard
        assert np.all(np.abs(opost[diff]) <= SAT_ATOL), (iters, int(diff.sum()), stats)
        if early_stop:
            assert np.mean(its == oits) >= 0.98, stats
        else:
            assert np.all(its == iters)


# ----------------------------------------- more codewords than workgroups
@pytest.mark.parametrize("name", ["r432_12288", "r48_9216"])
def test_more_codewords_than_workgroups(torch, name):
    """B = 264 on kernels whose grid is capped at 256 workgroups with one slab each: eight
    workgroups decode a second codeword on the slab (and LDS) their first one used."""
    g, csr = _case(name)
    frames = 264
    calls = [(1, 0, 0, 1, 3, frames), (1, 1, 0, 1, 20, frames), (0, 0, 0, 1, 3, frames)]
    for p in _routed(name, calls):
        assert p["grid"] == 256 and p["slab"] > 0, p
    llr = _awgn(g.n, 0.90, 22, frames)
    for iters, early_stop in ((3, False), (20, True)):
        post, hard, its = _decode(g, llr, iters, "minsum", 0.75, early_stop)
        opost, ohard, oits = oracle.bp_decode_batch(csr, llr, iters, 1, 0.75, early_stop)
        np.testing.assert_array_equal(hard, ohard)
        np.testing.assert_array_equal(its, oits)
        np.testing.assert_array_equal(post, opost)
    post, hard, its = _decode(g, llr, 3, "spa")
    opost, ohard, _ = oracle.bp_decode_batch(csr, llr, 3, 0)
    stats = {"graph": name, "kernel": FALLBACK_KERNELS[name], "frames": frames, "iters3": _spa_margins(post, opost),
             "second_pass_frames": _spa_margins(post[256:], opost[256:])}
    _dump("fallback_spa_b264_" + name, stats)
    np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL, err_msg=str(stats))


# --------------------------------------------------------------- Monte-Carlo
MC_B, MC_ITERS = 128, 20


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name,p", [("r58_320", 0.07), ("r324_1024", 0.01), ("mixA", 0.12)])
def test_mc_minsum_bsc_exact(torch, name, p, early_stop):
    """Counters built from the oracle as tests/test_gpu_parity.py::test_mc_minsum_bsc_exact does:
    frames, frame / bit errors, iterations and the per-iteration error curve, all bit-exact."""
    g, csr = _case(name)
    _routed(name, [(1, int(early_stop), 1, 0, MC_ITERS, MC_B)])
    got = _mc_counters(g, "bsc", p, 8, MC_B, MC_ITERS, "minsum", 0.75, early_stop)
    llr = oracle.channel(oracle.CH_BSC, p, 8, 0, g.n, MC_B)
    want = np.zeros(4 + MC_ITERS + 1, np.int64)
    want[0] = MC_B
    want[4] = int((llr < 0).sum())
    for t in range(1, MC_ITERS + 1):
        _, h, _ = oracle.bp_decode_batch(csr, llr, t, 1, alpha=0.75, early_stop=early_stop)
        want[4 + t] = int(h.sum())
    _, h, its = oracle.bp_decode_batch(csr, llr, MC_ITERS, 1, alpha=0.75, early_stop=early_stop)
    want[1] = int(h.any(axis=1).sum())
    want[2] = int(h.sum())
    want[3] = int(its.sum())
    assert 0 < want[1] < MC_B  # both decoded and failed frames
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name,sigma", [("r510_640", 0.77), ("mixA", 1.05)])
def test_mc_spa_awgn_vs_oracle(torch, name, sigma, early_stop):
    """Tolerances of tests/test_gpu_loc.py::test_loc_mc_spa_vs_oracle.  A NaN posterior counts as
    no error (s < 0 is false), so the unscaled check rule reported zero frame errors here."""
    g, csr = _case(name)
    _routed(name, [(0, int(early_stop), 1, 0, MC_ITERS, MC_B)])
    got = _mc_counters(g, "awgn", sigma, 31, MC_B, MC_ITERS, "spa", 1.0, early_stop)
    llr = oracle.channel(oracle.CH_AWGN, sigma, 31, 0, g.n, MC_B)
    _, h, its = oracle.bp_decode_batch(csr, llr, MC_ITERS, 0, early_stop=early_stop)
    fe, be, ti = int(h.any(axis=1).sum()), int(h.sum()), int(its.sum())
    _dump("fallback_mc_spa_%s_%s" % (name, "es" if early_stop else "fixed"),
          {"graph": name, "kernel": FALLBACK_KERNELS[name], "sigma": sigma, "counters_gpu": got[:4].tolist(),
           "counters_oracle": [MC_B, fe, be, ti]})
    assert 0 < fe < MC_B  # both decoded and failed frames at this sigma
    assert got[0] == MC_B
    assert abs(int(got[1]) - fe) <= 2, (got[:4], fe, be, ti)
    assert abs(int(got[2]) - be) <= 0.02 * be + 20, (got[:4], fe, be)
    assert abs(int(got[3]) - ti) <= 0.005 * ti + 2, (got[:4], ti)
    assert got[4] == int((llr < 0).sum())  # channel errors: bit-exact (Philox + fused channel)
    assert got[4 + MC_ITERS] == got[2]  # the last curve point is the final error count
