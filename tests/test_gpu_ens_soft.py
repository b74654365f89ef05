"""Soft decoding over the random (dv, dc) ensemble (csrc/bp_ens.hip) against the oracle: word /
trial b decodes on graph b of the device sampler, with no host-built layout.

The oracle of trial b is sample_regular(n, dv, dc, seed, b) -> csr_from_lists ->
bp_decode_batch(csr, llr[b:b+1]), with llr = oracle.channel(kind, p, seed, 0, n, B) (graph and
channel word share the key, as the Monte-Carlo entry draws them).  Shapes:
  (3,6) n = 200   B = 264  LDS form, one-level sampler, more words than the 256 workgroups;
  (3,9) n = 90    B = 48   the MAXDC = 16 bucket and the check rule of degrees above 6;
  (3,6) n = 10,000 B = 6   slab form, sequential-draw sampler;
  (5,10) n = 120  B = 8    variable degree above 4 (the looped variable branch), on caller-owned
                           lists from tests.graph_util.regular_simple.
Min-sum (alpha = 0.75) is held bit-exact -- decisions, iteration counts, posteriors, every
Monte-Carlo counter and the whole error curve; sum-product to the project's unsaturated tolerance
(tests/test_gpu_fallback.py) at a sigma whose oracle posteriors stay under the message clamp.
Each test first asserts what its inputs are claimed to be on the oracle side, and holds its call
to the kernel name the plan gives (ldpc_debug_ens_plan).
"""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests.test_ens_plan import ens_plans
from tests.test_gpu_fullsize import _dump

pytestmark = pytest.mark.gpu

SPA_ATOL, SPA_RTOL = 1e-4, 1e-4   # tests/test_gpu_fallback.py
XMAX = 23 * np.log(2.0)           # the message clamp (oracle ORACLE_XMAX)
ALPHA = 0.75
KERNEL = {(200, 3, 6): "bp_ens_kernel<8,lds>", (90, 3, 9): "bp_ens_kernel<16,lds>",
          (10000, 3, 6): "bp_ens_kernel<8,gmem>"}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


# ------------------------------------------------------------------- oracle
@functools.lru_cache(maxsize=None)
def _csrs(n, dv, dc, seed, B):
    """CSR slot form of graphs 0 .. B-1 of the sampler's restatement, and the two list batches."""
    chk, var, att = oracle.sample_regular_batch(n, dv, dc, seed, 0, B)
    assert np.all(att > 0)
    m = n * dv // dc
    return [oracle.csr_from_lists(var[b], chk[b], n, m, dv, dc) for b in range(B)], chk, var


@functools.lru_cache(maxsize=None)
def _llr(kind, p, seed, n, B):
    llr = oracle.channel(kind, p, seed, 0, n, B)
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def _oracle(shape, kind, p, seed, B, iters, algo, early_stop):
    """(post, hard, its) of the B words, word b on graph b."""
    n = shape[0]
    csrs = _csrs(*shape, seed, B)[0]
    llr = _llr(kind, p, seed, n, B)
    post, hard, its = np.zeros((B, n), np.float32), np.zeros((B, n), np.uint8), np.zeros(B, np.int32)
    for b in range(B):
        po, ha, it = oracle.bp_decode_batch(csrs[b], llr[b:b + 1], iters, algo, ALPHA if algo == 1 else 1.0, early_stop)
        post[b], hard[b], its[b] = po[0], ha[0], it[0]
    return post, hard, its


@functools.lru_cache(maxsize=None)
def _oracle_trials(shape, p, seed, B, iters, early_stop):
    """Min-sum on the BSC: per-trial error curves [B][iters + 1] (one oracle decode per iteration
    count, as tests/test_gpu_parity.py::test_mc_minsum_bsc_exact builds its curve) and iteration
    counts [B]."""
    llr = _llr(oracle.CH_BSC, p, seed, shape[0], B)
    curve = np.zeros((B, iters + 1), np.int64)
    curve[:, 0] = (llr < 0).sum(axis=1)
    for t in range(1, iters + 1):
        curve[:, t] = _oracle(shape, oracle.CH_BSC, p, seed, B, t, 1, early_stop)[1].sum(axis=1)
    return curve, _oracle(shape, oracle.CH_BSC, p, seed, B, iters, 1, early_stop)[2].astype(np.int64)


def _counters(curve, its, X=-1, stop=0):
    """The sequential trial loop (parallel_simulator.py:198, expurgated :238): a trial counts its
    frame / bit errors and curve when its final error count is > X; the loop ends with the trial
    that brings the counted frame errors to `stop`."""
    iters = curve.shape[1] - 1
    want = np.zeros(4 + iters + 1, np.int64)
    for row, it in zip(curve, its):
        want[0] += 1
        want[3] += it
        if row[-1] > X:
            want[1] += row[-1] != 0
            want[2] += row[-1]
            want[4:] += row
        if stop and want[1] >= stop:
            break
    return want


# ------------------------------------------------------------------- device
def _routed(shape, calls):
    """Every call (algo, early_stop, mc, want_post, iters, B) runs the kernel this module names."""
    rc, plans = ens_plans(*shape, calls)
    assert rc == 0
    for call, p in zip(calls, plans):
        assert p["name"] == KERNEL[shape], (shape, call, p)
        assert p["grid"] == min(call[5], 256), (shape, call, p)
    return plans


@functools.lru_cache(maxsize=None)
def _device_graphs(shape, seed, B):
    """Graphs 0 .. B-1 from ldpc_sample_regular_dev, checked against the oracle's once."""
    import torch
    from iib_project_ldpc_codes_amd import _native
    n, dv, dc = shape
    chk = torch.zeros((B, n * dv), dtype=torch.int32, device="cuda")
    var = torch.zeros((B, n * dv), dtype=torch.int32, device="cuda")
    rc = _native.lib().ldpc_sample_regular_dev(n, dv, dc, seed, 0, B, chk.data_ptr(), var.data_ptr(), None,
                                               torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "ldpc_sample_regular_dev")
    torch.cuda.synchronize()
    _, ochk, ovar = _csrs(n, dv, dc, seed, B)
    np.testing.assert_array_equal(chk.cpu().numpy(), ochk)
    np.testing.assert_array_equal(var.cpu().numpy(), ovar)
    return chk, var


def _decode(shape, seed, llr, iters, algo, early_stop, want_post=True):
    import torch
    from iib_project_ldpc_codes_amd import decoder
    chk, var = _device_graphs(shape, seed, llr.shape[0])
    lists = chk.clone(), var.clone()
    post, hard, its = decoder.bp_ensemble_decode_dev(*shape, lists[0], lists[1], torch.from_numpy(np.array(llr)).cuda(),
                                                     iters, algo, ALPHA if algo == "minsum" else 1.0, early_stop,
                                                     want_post=want_post)
    torch.cuda.synchronize()
    assert torch.equal(lists[0], chk) and torch.equal(lists[1], var)  # caller-owned lists are only read
    return None if post is None else post.cpu().numpy(), hard.cpu().numpy(), its.cpu().numpy()


def _mc(shape, channel, p, seed, B, iters, algo, early_stop, X=-1, stop=0):
    import torch
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    mc = MonteCarlo.ensemble(*shape, channel, p, iters, algo=algo, alpha=ALPHA if algo == "minsum" else 1.0,
                             early_stop=early_stop, seed=seed, batch=B, expurgation=X)
    mc.run_batch(0, B, stop)
    torch.cuda.synchronize()
    return mc.counters.cpu().numpy()


# ------------------------------------------------- 1. decode entry, min-sum
MS_CASES = [((200, 3, 6), 264, 0.06, 17), ((90, 3, 9), 48, 0.03, 17), ((10000, 3, 6), 6, 0.07, 5),
            ((10000, 3, 6), 6, 0.08, 5)]


@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("shape,B,p,seed", MS_CASES)
def test_decode_minsum_bit_exact(torch, shape, B, p, seed, early_stop):
    if shape[0] == 10000:  # the oracle decodes every frame at 0.07 and none at 0.08
        failed = _oracle(shape, oracle.CH_BSC, p, seed, B, 20, 1, early_stop)[1].any(axis=1).sum()
        assert failed == (0 if p == 0.07 else B)
    _routed(shape, [(1, int(early_stop), 0, 1, it, B) for it in (1, 3, 20)])
    llr = _llr(oracle.CH_BSC, p, seed, shape[0], B)
    for iters in (1, 3, 20):
        post, hard, its = _decode(shape, seed, llr, iters, "minsum", early_stop)
        opost, ohard, oits = _oracle(shape, oracle.CH_BSC, p, seed, B, iters, 1, early_stop)
        np.testing.assert_array_equal(hard, ohard)
        np.testing.assert_array_equal(its, oits)
        np.testing.assert_array_equal(post, opost)


@pytest.mark.parametrize("shape,B,p,seed", MS_CASES[:3])
def test_decode_null_posteriors_zero_iterations_empty_batch(torch, shape, B, p, seed):
    from iib_project_ldpc_codes_amd import decoder
    _routed(shape, [(1, 1, 0, 0, 20, B), (1, 0, 0, 1, 0, B)])
    llr = _llr(oracle.CH_BSC, p, seed, shape[0], B)
    # d_post = NULL, early stop: the same decisions and counts
    post, hard, its = _decode(shape, seed, llr, 20, "minsum", True, want_post=False)
    _, ohard, oits = _oracle(shape, oracle.CH_BSC, p, seed, B, 20, 1, True)
    assert post is None
    np.testing.assert_array_equal(hard, ohard)
    np.testing.assert_array_equal(its, oits)
    # max_iters = 0: the LLRs come back
    post, hard, its = _decode(shape, seed, llr, 0, "minsum", False)
    np.testing.assert_array_equal(post, llr)
    np.testing.assert_array_equal(hard, llr < 0)
    assert np.all(its == 0)
    # B = 0: a no-op on empty tensors
    n, dv, dc = shape
    empty = torch.empty((0, n * dv), dtype=torch.int32, device="cuda")
    post, hard, its = decoder.bp_ensemble_decode_dev(n, dv, dc, empty, empty,
                                                     torch.empty((0, n), dtype=torch.float32, device="cuda"), 20,
                                                     "minsum", ALPHA)
    torch.cuda.synchronize()
    assert post.shape == (0, n) and its.numel() == 0


@pytest.mark.parametrize("early_stop", [False, True])
def test_decode_minsum_variable_degree_5_bit_exact(torch, early_stop):
    """Variable degree 5 > 4: the looped variable branch.  The configuration model almost never
    draws a simple (5,10) graph, so the eight graphs are tests.graph_util.regular_simple's (lists
    in the sampler's format) handed to the decode entry as caller-owned lists."""
    from iib_project_ldpc_codes_amd import decoder
    from tests.graph_util import regular_simple
    shape, B = (120, 5, 10), 8
    n, dv, dc = shape
    rc, plans = ens_plans(*shape, [(1, int(early_stop), 0, 1, it, B) for it in (1, 3, 20)])
    assert rc == 0 and all(p["name"] == "bp_ens_kernel<16,lds>" for p in plans)
    graphs = [regular_simple(n, dv, dc, seed=40 + b) for b in range(B)]
    chk = torch.from_numpy(np.stack([g.check_lookup for g in graphs]).astype(np.int32)).cuda()
    var = torch.from_numpy(np.stack([g.variable_lookup for g in graphs]).astype(np.int32)).cuda()
    llr = _llr(oracle.CH_BSC, 0.04, 9, n, B)
    failed = 0
    for iters in (1, 3, 20):
        post, hard, its = decoder.bp_ensemble_decode_dev(n, dv, dc, chk, var, torch.from_numpy(np.array(llr)).cuda(),
                                                         iters, "minsum", ALPHA, early_stop)
        torch.cuda.synchronize()
        for b, g in enumerate(graphs):
            csr = oracle.csr_from_lists(g.variable_lookup, g.check_lookup, n, g.m, dv, dc)
            opost, ohard, oits = oracle.bp_decode_batch(csr, llr[b:b + 1], iters, 1, ALPHA, early_stop)
            np.testing.assert_array_equal(hard[b].cpu().numpy(), ohard[0])
            np.testing.assert_array_equal(post[b].cpu().numpy(), opost[0])
            assert int(its[b]) == int(oits[0])
            failed += int(ohard.any()) if iters == 20 else 0
    assert 0 < failed < B  # decoded and failed frames among the eight


# --------------------------------------------- 2. decode entry, sum-product
@pytest.mark.parametrize("shape,B,sigma", [((200, 3, 6), 24, 0.95), ((90, 3, 9), 24, 0.80), ((10000, 3, 6), 4, 0.95)])
def test_decode_spa_unsaturated_posterior_tolerance(torch, shape, B, sigma):
    seed = 21
    _routed(shape, [(0, 0, 0, 1, it, B) for it in (1, 3, 5)])
    llr = _llr(oracle.CH_AWGN, sigma, seed, shape[0], B)
    stats = {"shape": list(shape), "kernel": KERNEL[shape], "sigma": sigma, "frames": B}
    got = {}
    for iters in (1, 3, 5):
        opost, ohard, _ = _oracle(shape, oracle.CH_AWGN, sigma, seed, B, iters, 0, False)
        assert np.abs(opost).max() < XMAX  # the case is what it claims: nothing at the clamp
        post, hard, its = _decode(shape, seed, llr, iters, "spa", False)
        d = np.abs(post.astype(np.float64) - opost)
        tol = SPA_ATOL + SPA_RTOL * np.abs(opost.astype(np.float64))
        stats["iters%d" % iters] = {"post_max_abs": float(np.nanmax(d)), "oracle_post_max_abs": float(np.abs(opost).max()),
                                    "oracle_post_max_over_clamp": float(np.abs(opost).max() / XMAX),
                                    "max_err_over_tol": float(np.nanmax(d / tol)), "nan_count": int(np.isnan(post).sum()),
                                    "decisions_differ": int((hard != ohard).sum())}
        got[iters] = (post, hard, its, opost, ohard, tol)
    _dump("ens_spa_unsat_n%d_dc%d" % (shape[0], shape[2]), stats)
    for iters, (post, hard, its, opost, ohard, tol) in got.items():
        np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL, err_msg=str(stats))
        sure = np.abs(opost) > tol
        np.testing.assert_array_equal(hard[sure], ohard[sure])
        assert np.all(its == iters)


# --------------------------------------------- 3. Monte-Carlo, min-sum, BSC
MC_ITERS = 20
MC_CASES = [((200, 3, 6), 264, 0.06, 17, 61), ((90, 3, 9), 48, 0.03, 17, 11), ((10000, 3, 6), 6, 0.08, 5, 6)]


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("shape,B,p,seed,fe", MC_CASES)
def test_mc_minsum_bsc_exact(torch, shape, B, p, seed, fe, early_stop):
    curve, its = _oracle_trials(shape, p, seed, B, MC_ITERS, early_stop)
    want = _counters(curve, its)
    assert want[1] == fe and want[0] == B  # the oracle's own frame errors on these trials
    if shape[0] == 200:
        assert 5 <= want[1] <= B - 5
        assert sorted(curve[:, -1][curve[:, -1] > 0])[:8] == [2, 2, 3, 3, 3, 4, 4, 5]
    _routed(shape, [(1, int(early_stop), 1, 0, MC_ITERS, B)])
    got = _mc(shape, "bsc", p, seed, B, MC_ITERS, "minsum", early_stop)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("X,stop", [(3, 0), (-1, 5), (3, 5)])
def test_mc_minsum_bsc_expurgation_and_stop_rule(torch, X, stop, early_stop):
    """(3,6) n = 200: X = 3 drops the five failed frames with <= 3 residual errors; the stop rule
    cuts the batch at the fifth counted frame error, which with X = 3 is a later trial."""
    shape, B, p, seed, _ = MC_CASES[0]
    curve, its = _oracle_trials(shape, p, seed, B, MC_ITERS, early_stop)
    plain, want = _counters(curve, its), _counters(curve, its, X, stop)
    last = curve[:, -1]
    assert ((last > 0) & (last <= 3)).sum() == 5
    if stop:
        assert want[1] == stop and want[0] < B
        if X == 3:
            assert want[0] > _counters(curve, its, -1, stop)[0]
    else:
        assert want[1] == plain[1] - 5 and want[0] == B
    _routed(shape, [(1, int(early_stop), 1, 0, MC_ITERS, B)])
    got = _mc(shape, "bsc", p, seed, B, MC_ITERS, "minsum", early_stop, X, stop)
    np.testing.assert_array_equal(got, want)


# ------------------------------------------- 4. Monte-Carlo, sum-product, AWGN
@pytest.mark.parametrize("early_stop", [True, False])
def test_mc_spa_awgn_vs_oracle(torch, early_stop):
    """Tolerances of tests/test_gpu_loc.py::test_loc_mc_spa_vs_oracle."""
    shape, B, sigma, seed, iters = (200, 3, 6), 96, 0.8, 31, 20
    _, h, its = _oracle(shape, oracle.CH_AWGN, sigma, seed, B, iters, 0, early_stop)
    fe, be, ti = int(h.any(axis=1).sum()), int(h.sum()), int(its.sum())
    assert 0 < fe < B and fe == 26
    _routed(shape, [(0, int(early_stop), 1, 0, iters, B)])
    got = _mc(shape, "awgn", sigma, seed, B, iters, "spa", early_stop)
    _dump("ens_mc_spa_n200_%s" % ("es" if early_stop else "fixed"),
          {"kernel": KERNEL[shape], "sigma": sigma, "counters_gpu": got[:4].tolist(), "counters_oracle": [B, fe, be, ti]})
    llr = _llr(oracle.CH_AWGN, sigma, seed, shape[0], B)
    assert got[0] == B
    assert got[4] == int((llr < 0).sum())  # channel errors: bit-exact (Philox + fused channel)
    assert abs(int(got[1]) - fe) <= 2, (got[:4], fe, be, ti)
    assert abs(int(got[2]) - be) <= 0.02 * be + 20, (got[:4], fe, be)
    assert abs(int(got[3]) - ti) <= 0.005 * ti + 2, (got[:4], ti)
    assert got[4 + iters] == got[2]  # the last curve point is the final error count


# ------------------------------------------------------------- 5. ldpc_mc_run
def test_mc_run_ensemble_bsc_equals_montecarlo(torch):
    """ldpc_mc_run with NULL lists on the BSC: the counters of MonteCarlo.ensemble over the same 150
    trials (the pattern of tests/test_gpu_multirank.py::test_mc_run_num_tests_clamp_and_ensemble);
    the BEC ensemble call still gives what the BEC entry gives."""
    from iib_project_ldpc_codes_amd import montecarlo
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    shape = (200, 3, 6)
    _routed(shape, [(1, 1, 1, 0, 20, 96), (1, 1, 1, 0, 20, 54)])
    got = montecarlo.mc_run(("ensemble",) + shape, "bsc", 0.06, 20, algo="minsum", alpha=ALPHA, devices=(0,),
                            num_tests=150, stop_frame_errors=0, seed=17, batch=96)
    ref = MonteCarlo.ensemble(*shape, "bsc", 0.06, 20, algo="minsum", alpha=ALPHA, seed=17, batch=96)
    ref.run_batch(0, 96)
    ref.run_batch(96, 54)
    torch.cuda.synchronize()
    want = ref.counters.cpu().numpy()
    assert got["num_tests"] == 150 and 0 < want[1] < 150
    np.testing.assert_array_equal(got["raw_counters"], want)
    curve, its = _oracle_trials(shape, 0.06, 17, 264, MC_ITERS, True)  # the trials of MC_CASES[0]
    np.testing.assert_array_equal(want, _counters(curve[:150], its[:150]))
    bec = montecarlo.mc_run(("ensemble",) + shape, "bec", 0.40, 20, devices=(0,), num_tests=150, stop_frame_errors=0,
                            seed=17, batch=96, expurgation=1)
    mce = MonteCarlo.ensemble(*shape, "bec", 0.40, 20, seed=17, batch=96, expurgation=1)
    mce.run_batch(0, 96)
    mce.run_batch(96, 54)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bec["raw_counters"], mce.counters.cpu().numpy())
    chk, var, _ = oracle.sample_regular_batch(*shape, 17, 0, 150)
    words = oracle.channel(oracle.CH_BEC, 0.40, 17, 0, 200, 150)
    rows, bits = [], []
    for t in range(150):
        _, err, it = oracle.message_passing(words[t], 20, var[t], chk[t], 200, 100, 3, 6)
        rows.append(np.insert(err, 0, int(np.count_nonzero(words[t] == 2))))
        bits.append(it)
    np.testing.assert_array_equal(bec["raw_counters"], _counters(np.array(rows, np.int64), np.array(bits), X=1))
