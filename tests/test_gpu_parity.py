"""GPU parity: the HIP path (through the C ABI) against the oracle / the reference's golden vectors.

Tolerances (stated):
  * BEC decoding, BEC/BSC channels, min-sum decoding, MC counters: bit-exact.
  * Sum-product posteriors: the kernel uses the hardware exp/log/rcp
    (v_exp_f32 / v_log_f32 / v_rcp_f32, ~1 ulp) where the oracle uses libm and
    IEEE division; per-message error ~1e-6 relative.  After 1-5 iterations
    |post_gpu - post_cpu| <= 1e-4 + 1e-4 |post_cpu| (SPA_ATOL/SPA_RTOL); after
    many iterations trajectories can separate on frames near a decision boundary,
    so 50-iteration runs compare hard decisions (>= 98 % of frames identical)
    and FER within sampling noise.  Early-stopped high-SNR frames (saturated
    messages, |post| ~ 60 nats): >= 99.9 % of values within SPA_ATOL/SPA_RTOL,
    all within SAT_ATOL + SAT_RTOL |post_cpu| (the check rule's D - N cancellation).
  * BI-AWGN channel LLRs: |d| <= 1e-5 (1 + |llr|) (hardware log/sin/cos vs libm).
"""
import ctypes as ct

import numpy as np
import pytest

from oracle import oracle
from tests.golden_util import load_bec_golden
from tests.graph_util import BEC_DECODE, BEC_MC, bec_plans

pytestmark = pytest.mark.gpu

SPA_ATOL = 1e-4
SPA_RTOL = 1e-4
SAT_ATOL = 1e-3   # sum-product posteriors of converged high-SNR frames (saturated messages)
SAT_RTOL = 3e-3


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


@pytest.fixture(scope="module")
def lib():
    from iib_project_ldpc_codes_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def golden():
    return load_bec_golden()


def _graph(golden, gi):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    n, k, dv, dc, v2c, c2v = golden[0][gi]
    return TannerGraph(v2c, c2v, n, k, dv, dc)


# --------------------------------------------------------------------- BEC
def test_dropin_message_passing_matches_reference_golden(lib, golden):
    """libldpc_mi355x.so:message_passing driven exactly as parallel_simulator.py:145-165."""
    graphs, cases = golden
    for c in cases:
        n, k, dv, dc, v2c, c2v = graphs[c["gi"]]
        if n > 1000:
            continue
        word = np.array(c["word"], dtype="int32")
        errors = np.zeros(c["max_its"], np.int32) if c["errin"] is None else c["errin"].astype(np.int32).copy()
        v2c_ = np.ascontiguousarray(v2c, np.int32)
        c2v_ = np.ascontiguousarray(c2v, np.int32)
        it = lib.message_passing(word.ctypes.data, c["max_its"], v2c_.ctypes.data, c2v_.ctypes.data,
                                 errors.ctypes.data, n, k, dv, dc)
        assert it == c["it"], (c["gi"], c["max_its"])
        np.testing.assert_array_equal(word.astype(np.int8), c["out"])
        if c["errin"] is None:
            errors = np.insert(errors, 0, int(np.count_nonzero(c["word"] == 2)))
        np.testing.assert_array_equal(errors, c["errors"])


def test_dropin_message_passing_graph_changes(lib, golden):
    """The drop-in's graph cache across code changes: the golden cases in a shuffled order, so
    consecutive calls switch between codes of the same shape (the ensemble loop's new code per
    trial, parallel_simulator.py:198-223: device arrays refilled in place) and of other shapes
    (graph rebuilt), every list a fresh copy; each call still equals the reference's output."""
    graphs, cases = golden
    cs = [c for c in cases if graphs[c["gi"]][0] <= 1000]
    assert len({c["gi"] for c in cs}) >= 2
    order = np.random.default_rng(7).permutation(len(cs))
    for j in order:
        c = cs[j]
        n, k, dv, dc, v2c, c2v = graphs[c["gi"]]
        word = np.array(c["word"], dtype="int32")
        errors = np.zeros(c["max_its"], np.int32) if c["errin"] is None else c["errin"].astype(np.int32).copy()
        v2c_ = np.array(v2c, np.int32)
        c2v_ = np.array(c2v, np.int32)
        it = lib.message_passing(word.ctypes.data, c["max_its"], v2c_.ctypes.data, c2v_.ctypes.data,
                                 errors.ctypes.data, n, k, dv, dc)
        assert it == c["it"], (c["gi"], c["max_its"])
        np.testing.assert_array_equal(word.astype(np.int8), c["out"])
        if c["errin"] is None:
            errors = np.insert(errors, 0, int(np.count_nonzero(c["word"] == 2)))
        np.testing.assert_array_equal(errors, c["errors"])


def test_dropin_message_passing_same_shape_codes_alternate(lib):
    """Two (3,6) n = 1000 codes of one shape, alternating call by call (the ensemble loop's new
    code per trial re-sent through message_passing): the device arrays are refilled in place
    and every call equals the oracle's message_passing.c restatement on its own code."""
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from oracle import oracle
    codes = [TannerGraph.random_regular(1000, 3, 6, seed=s) for s in (21, 22)]
    rng = np.random.default_rng(5)
    for call in range(12):
        g = codes[call % 2]
        word = np.where(rng.random(g.n) < 0.42, 2, 0).astype(np.int32)
        want_w, want_e, want_it = oracle.bec_decode_batch(word[None, :], 50, g.variable_lookup, g.check_lookup,
                                                          g.n, g.k, 3, 6)
        errors = np.zeros(50, np.int32)
        v2c, c2v = np.array(g.variable_lookup, np.int32), np.array(g.check_lookup, np.int32)
        it = lib.message_passing(word.ctypes.data, 50, v2c.ctypes.data, c2v.ctypes.data, errors.ctypes.data,
                                 g.n, g.k, 3, 6)
        assert it == want_it[0], call
        np.testing.assert_array_equal(word.astype(np.int8), want_w[0])
        np.testing.assert_array_equal(errors, want_e[0])


def test_bec_batch_matches_reference_golden(golden):
    from iib_project_ldpc_codes_amd import decoder
    graphs, cases = golden
    groups = {}
    for c in cases:
        if c["errin"] is None:
            groups.setdefault((c["gi"], c["max_its"]), []).append(c)
    for (gi, max_its), cs in groups.items():
        g = _graph(golden, gi)
        words = np.stack([c["word"] for c in cs]).astype(np.uint8)
        w, err, its = decoder.bec_decode(g, words, max_its)
        for b, c in enumerate(cs):
            np.testing.assert_array_equal(w[b].astype(np.int8), c["out"])
            np.testing.assert_array_equal(err[b], c["errors"][1:])
            assert its[b] == c["it"]


def test_bec_batch_caller_errors_accumulate(golden):
    from iib_project_ldpc_codes_amd import decoder
    graphs, cases = golden
    for c in [c for c in cases if c["errin"] is not None]:
        g = _graph(golden, c["gi"])
        w, err, its = decoder.bec_decode(g, c["word"][None].astype(np.uint8), c["max_its"], errors=c["errin"][None])
        np.testing.assert_array_equal(err[0], c["errors"])
        assert its[0] == c["it"]


def test_bec_large_batch_vs_oracle(torch):
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(10000, 3, 6, seed=7)
    words = oracle.channel(oracle.CH_BEC, 0.42, 99, 0, g.n, 48)
    w, err, its = decoder.bec_decode(g, words.astype(np.uint8), 50)
    ow, oerr, oits = oracle.bec_decode_batch(words, 50, g.variable_lookup, g.check_lookup, g.n, g.k, 3, 6)
    np.testing.assert_array_equal(w.astype(np.int8), ow)
    np.testing.assert_array_equal(err, oerr)
    np.testing.assert_array_equal(its, oits)


def test_bec_irregular_csr_vs_oracle(torch):
    """CSR graph through ldpc_graph_create_csr; oracle on the equivalent lists."""
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g0 = TannerGraph.random_regular(600, 3, 6, seed=3)
    g = TannerGraph.from_csr(*g0.to_csr())
    words = oracle.channel(oracle.CH_BEC, 0.45, 5, 0, g.n, 16)
    w, err, its = decoder.bec_decode(g, words.astype(np.uint8), 30)
    ow, oerr, oits = oracle.bec_decode_batch(words, 30, g0.variable_lookup, g0.check_lookup, 600, 300, 3, 6)
    np.testing.assert_array_equal(w.astype(np.int8), ow)
    np.testing.assert_array_equal(err, oerr)
    np.testing.assert_array_equal(its, oits)


# Batches of >= 64 words run on bec_dec_bits_kernel (16 words per u32 plane
# word, or 4 per byte for graphs whose u32 planes do not fit LDS).
def test_bec_bitsliced_batch_reference_golden(golden):
    """Every reference golden case (with and without caller errors[]), tiled to
    130 words per (graph, max_its) so the batch takes the bit-sliced kernel with
    a partial last workgroup; outputs must equal message_passing.c's."""
    from iib_project_ldpc_codes_amd import decoder
    graphs, cases = golden
    groups = {}
    for c in cases:
        groups.setdefault((c["gi"], c["max_its"]), []).append(c)
    for (gi, max_its), cs in groups.items():
        g = _graph(golden, gi)
        rows = [cs[i % len(cs)] for i in range(130)]
        words = np.stack([c["word"] for c in rows]).astype(np.uint8)
        errin = np.stack([np.zeros(max_its, np.int32) if c["errin"] is None else c["errin"].astype(np.int32)
                          for c in rows])
        w, err, its = decoder.bec_decode(g, words, max_its, errors=errin)
        for b, c in enumerate(rows):
            np.testing.assert_array_equal(w[b].astype(np.int8), c["out"])
            np.testing.assert_array_equal(err[b], c["errors"][1:] if c["errin"] is None else c["errors"])
            assert its[b] == c["it"], (gi, max_its, b)


def _perturbed_bec_batch(n, B, eps, iters, seed):
    """Channel words with some rows corrupted (known bits flipped, so checks
    disagree and the last known message decides) and some rows given small
    caller errors[] that make the reference's stall test fire early."""
    rng = np.random.default_rng(seed)
    words = oracle.channel(oracle.CH_BEC, eps, seed, 0, n, B).astype(np.uint8)
    bad = rng.random((B, n)) < 0.002
    bad[::5] = False
    words[bad & (words != 2)] ^= 1
    errin = np.zeros((B, iters), np.int32)
    errin[::3] = rng.integers(0, 3, (len(errin[::3]), iters))
    return words, errin


# the last column, the kernel the plan names for the call, stays out of the test ids
BEC_BITS_CASES = [
    (1000, 65536, 0.42, 50, False, "bec_dec_bits_kernel<256,4,u32>"),
    (1000, 32768, 0.40, 20, False, "bec_dec_bits_kernel<256,2,u32>"),
    (1000, 130, 0.45, 50, True, "bec_dec_bits_kernel<256,1,u32>"),    # CSR graph, partial last workgroup
    (10000, 256, 0.42, 60, False, "bec_dec_bits_kernel<512,1,u32>"),
    (64800, 72, 0.42, 200, False, "bec_dec_bits_kernel<1024,1,u8>"),
]


@pytest.mark.parametrize("n,B,eps,iters,csr,kernel", BEC_BITS_CASES,
                         ids=["-".join(map(str, c[:-1])) for c in BEC_BITS_CASES])
def test_bec_bitsliced_batch_vs_oracle(torch, n, B, eps, iters, csr, kernel):
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    assert bec_plans(n, n // 2, [(BEC_DECODE, B, iters)])[0]["name"] == kernel
    g0 = TannerGraph.random_regular(n, 3, 6, seed=11)
    g = TannerGraph.from_csr(*g0.to_csr()) if csr else g0
    words, errin = _perturbed_bec_batch(n, B, eps, iters, seed=n + B)
    w, err, its = decoder.bec_decode(g, words, iters, errors=errin)
    ow, oerr, oits = oracle.bec_decode_batch(words, iters, g0.variable_lookup, g0.check_lookup, n, n // 2, 3, 6,
                                             errors=errin)
    np.testing.assert_array_equal(w.astype(np.int8), ow)
    np.testing.assert_array_equal(err, oerr)
    np.testing.assert_array_equal(its, oits)


# ----------------------------------------------------------------- channels
@pytest.mark.parametrize("n", [1000, 1003])
def test_channels_vs_oracle(torch, n):
    from iib_project_ldpc_codes_amd import decoder
    B, seed, first = 37, 0x1234_5678_9ABC, 5_000_000_000
    bec = decoder.channel_dev("bec", 0.4, seed, first, n, B).cpu().numpy()
    np.testing.assert_array_equal(bec.astype(np.int8), oracle.channel(oracle.CH_BEC, 0.4, seed, first, n, B))
    bsc = decoder.channel_dev("bsc", 0.07, seed, first, n, B).cpu().numpy()
    np.testing.assert_array_equal(bsc, oracle.channel(oracle.CH_BSC, 0.07, seed, first, n, B))
    awgn = decoder.channel_dev("awgn", 0.8, seed, first, n, B).cpu().numpy()
    ref = oracle.channel(oracle.CH_AWGN, 0.8, seed, first, n, B)
    assert np.all(np.abs(awgn - ref) <= 1e-5 * (1 + np.abs(ref)))


def test_channel_statistics(torch):
    from iib_project_ldpc_codes_amd import decoder
    x = decoder.channel_dev("bec", 0.3, 1, 0, 10000, 200).float()
    assert abs((x == 2).float().mean().item() - 0.3) < 0.003
    sigma = 0.9
    y = decoder.channel_dev("awgn", sigma, 2, 0, 10000, 100) * (sigma * sigma / 2.0)  # back to y
    assert abs(y.mean().item() - 1.0) < 0.005 and abs(y.std().item() - sigma) < 0.005


# --------------------------------------------------------------- soft paths
def _soft_case(n, B, sigma, seed, irregular=False):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g0 = TannerGraph.random_regular(n, 3, 6, seed=seed)
    csr = oracle.csr_from_lists(g0.variable_lookup, g0.check_lookup, n, g0.m, 3, 6)
    g = TannerGraph.from_csr(*csr) if irregular else g0
    llr = oracle.channel(oracle.CH_AWGN, sigma, seed, 0, n, B)
    return g, csr, llr


@pytest.mark.parametrize("irregular", [False, True])
@pytest.mark.parametrize("iters", [1, 2, 5])
def test_spa_posterior_tolerance(torch, iters, irregular):
    from iib_project_ldpc_codes_amd import decoder
    g, csr, llr = _soft_case(1000, 64, 0.85, 11, irregular)
    post, hard, its = decoder.bp_decode(g, llr, iters, "spa")
    opost, ohard, oits = oracle.bp_decode_batch(csr, llr, iters, 0)
    np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL)
    assert np.all(its == iters)


@pytest.mark.parametrize("irregular", [False, True])
def test_spa_50_iterations_hard_decisions(torch, irregular):
    from iib_project_ldpc_codes_amd import decoder
    g, csr, llr = _soft_case(1000, 256, 0.80, 12, irregular)
    post, hard, _ = decoder.bp_decode(g, llr, 50, "spa")
    opost, ohard, _ = oracle.bp_decode_batch(csr, llr, 50, 0)
    same = np.all(hard == ohard, axis=1)
    assert same.mean() >= 0.98  # chaotic frames near the decision boundary may separate
    fer_g = np.mean(hard.any(axis=1))
    fer_o = np.mean(ohard.any(axis=1))
    assert abs(fer_g - fer_o) <= 3 * np.sqrt(max(fer_o, 1 / 256) / 256)


@pytest.mark.parametrize("irregular", [False, True])
@pytest.mark.parametrize("early_stop", [False, True])
def test_minsum_bit_exact(torch, irregular, early_stop):
    from iib_project_ldpc_codes_amd import decoder
    g, csr, llr = _soft_case(1000, 64, 0.80, 13, irregular)
    post, hard, its = decoder.bp_decode(g, llr, 30, "minsum", alpha=0.75, early_stop=early_stop)
    opost, ohard, oits = oracle.bp_decode_batch(csr, llr, 30, 1, alpha=0.75, early_stop=early_stop)
    np.testing.assert_array_equal(post, opost)
    np.testing.assert_array_equal(hard, ohard)
    np.testing.assert_array_equal(its, oits)


@pytest.mark.parametrize("irregular", [False, True])
def test_early_stop_posteriors_more_frames_than_slabs(torch, irregular):
    """Early stop with posteriors on more frames than the persistent grids hold slabs for
    (B = 1,100 > 2 x 256 workgroups): the regular code runs bp_loc_kernel's slab path, the
    irregular one (min-sum early stop needs one check class there) falls back to another
    kernel.  The launchers refuse a scratch smaller than the path's layout, so a slab sizing
    that drifted from the dispatch fails here instead of writing past the buffer.  Min-sum:
    bit-exact against the oracle."""
    from iib_project_ldpc_codes_amd import decoder, ensembles
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    B = 1100
    if irregular:
        g = ensembles.sample_irregular(ensembles.RSU_DL4, 4000, seed=3, deg2="zigzag")
    else:
        g = TannerGraph.random_regular(1000, 3, 6, seed=14)
    csr = g.to_csr()
    llr = oracle.channel(oracle.CH_AWGN, 0.80, 15, 0, g.n, B)
    for algo, code, alpha in (("minsum", 1, 0.75), ("spa", 0, 1.0)):
        post, hard, its = decoder.bp_decode(g, llr, 30, algo, alpha=alpha, early_stop=True)
        opost, ohard, oits = oracle.bp_decode_batch(csr, llr, 30, code, alpha=alpha, early_stop=True)
        if code == 1:
            np.testing.assert_array_equal(post, opost)
            np.testing.assert_array_equal(its, oits)
        assert np.mean(np.all(hard == ohard, axis=1)) >= 0.98


@pytest.mark.parametrize("irregular", [False, True])
def test_early_stop_stops_only_on_codewords(torch, irregular):
    """Syndrome early stop: a frame that stops before max_iters must carry a valid
    codeword (for the regular distinct-column code the all-zero one; the irregular
    code has low-weight codewords a decoder can converge to).  Large batches at the
    headline shape (LDS-resident kernel) and on an irregular graph (generic kernel);
    this catches a hard-decision write racing with the syndrome read."""
    from iib_project_ldpc_codes_amd import decoder, ensembles
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = (ensembles.sample_irregular(ensembles.RSU_DL4, 4000, seed=2, deg2="zigzag") if irregular
         else TannerGraph.random_regular(10000, 3, 6, seed=1, distinct_columns=True))
    for algo, ch, p in (("minsum", "bsc", 0.05), ("spa", "awgn", 0.80)):
        llr = decoder.channel_dev(ch, p, 11, 0, g.n, 65536)
        _, hard, its = decoder.bp_decode_dev(g, llr, 50, algo, alpha=0.75 if algo == "minsum" else 1.0,
                                             early_stop=True, want_post=False)
        torch.cuda.synchronize()
        stopped = its < 50
        assert int(stopped.sum()) > 60000
        # syndrome of every stopped frame's decision (slot -> check via cptr)
        cptr, cvar, _, _ = g.to_csr()
        slot_check = torch.from_numpy(np.repeat(np.arange(g.m), np.diff(cptr))).cuda()
        bits = hard[stopped][:, torch.from_numpy(cvar.astype(np.int64)).cuda()].to(torch.int32)
        par = torch.zeros((bits.shape[0], g.m), dtype=torch.int32, device="cuda")
        par.index_add_(1, slot_check, bits)
        assert int((par % 2).sum()) == 0, algo
        if not irregular:  # no low-weight codewords here: stopped frames are error-free
            assert int(hard[stopped].sum()) == 0, algo


def test_minsum_early_stop_headline_bit_exact(torch):
    """Min-sum with early stop at n = 10000, 4096 frames: decisions and stop iterations
    identical to the oracle on every frame."""
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(10000, 3, 6, seed=1, distinct_columns=True)
    csr = g.to_csr()
    llr = decoder.channel_dev("bsc", 0.06, 12, 0, g.n, 4096)
    post, hard, its = decoder.bp_decode_dev(g, llr, 50, "minsum", alpha=0.75, early_stop=True)
    torch.cuda.synchronize()
    opost, ohard, oits = oracle.bp_decode_batch(csr, llr.cpu().numpy(), 50, 1, alpha=0.75, early_stop=True)
    np.testing.assert_array_equal(its.cpu().numpy(), oits)
    np.testing.assert_array_equal(hard.cpu().numpy(), ohard)
    np.testing.assert_array_equal(post.cpu().numpy(), opost)


def test_spa_early_stop_iterations(torch):
    from iib_project_ldpc_codes_amd import decoder
    g, csr, llr = _soft_case(1000, 128, 0.70, 14)
    post, hard, its = decoder.bp_decode(g, llr, 50, "spa", early_stop=True)
    opost, ohard, oits = oracle.bp_decode_batch(csr, llr, 50, 0, early_stop=True)
    assert np.mean(its == oits) >= 0.99
    assert np.mean(np.all(hard == ohard, axis=1)) >= 0.99


@pytest.mark.parametrize("n", [1000, 10000])
def test_spa_early_stop_posterior_tolerance(torch, n):
    """Early-stop posteriors (the LDS kernel forms them as L + log2(prod r) after the
    stop) against the oracle's, frame by frame, at high SNR where converged frames
    carry saturated messages (|post| up to ~60 nats).  There the check rule's D - N
    cancellation turns ulp-level differences into ~1e-3 relative on a few values
    (the log-domain kernel shows the same: 5 of 64,000 values beyond SPA_RTOL), so
    >= 99.9 % of values must meet SPA_RTOL / SPA_ATOL and all of them SAT_RTOL /
    SAT_ATOL.  (A wire formula (R - 1) / max(R, 1) that loses 1 - a to rounding
    fails this test on 17 % of values.)"""
    from iib_project_ldpc_codes_amd import decoder
    g, csr, llr = _soft_case(n, 64, 0.62, 16)
    post, hard, its = decoder.bp_decode(g, llr, 5, "spa", early_stop=True)
    opost, ohard, oits = oracle.bp_decode_batch(csr, llr, 5, 0, early_stop=True)
    assert np.mean(its < 5) > 0.5
    same = its == oits
    assert same.mean() >= 0.98
    close = np.isclose(post[same], opost[same], rtol=SPA_RTOL, atol=SPA_ATOL)
    assert close.mean() >= 0.999
    np.testing.assert_allclose(post[same], opost[same], rtol=SAT_RTOL, atol=SAT_ATOL)


def test_headline_shape_spa_vs_oracle(torch):
    """(3,6) n=10000 (the bench workload's code) on a small batch."""
    from iib_project_ldpc_codes_amd import decoder
    g, csr, llr = _soft_case(10000, 8, 0.85, 15)
    assert g.kernel_name() in ("bp_loc_kernel", "bp_lds_kernel<3,6>")
    post, hard, its = decoder.bp_decode(g, llr, 3, "spa")
    opost, _, _ = oracle.bp_decode_batch(csr, llr, 3, 0)
    np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL)


def test_headline_full_batch_properties(torch):
    """B = 65536, n = 10000, 50 iterations (the bench step) -- size-independent checks:
    deterministic across runs; at sigma = 0.70 (Eb/N0 ~ 3.1 dB) FER is small (this
    configuration-model code has a weight-2 codeword -- duplicate columns are allowed
    by random_code_generator.c -- so the floor is not zero); sampled frames, including
    failing ones, agree with the oracle."""
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(10000, 3, 6, seed=1)
    llr = decoder.channel_dev("awgn", 0.70, 3, 0, g.n, 65536)
    _, hard, its = decoder.bp_decode_dev(g, llr, 50, "spa", want_post=False)
    _, hard2, _ = decoder.bp_decode_dev(g, llr, 50, "spa", want_post=False)
    torch.cuda.synchronize()
    assert torch.equal(hard, hard2)
    assert int(its.min().item()) == 50
    errs = hard.sum(dim=1).cpu().numpy()
    assert np.mean(errs > 0) < 0.1
    bad = np.nonzero(errs)[0][:4]
    pick = np.concatenate([bad, np.arange(4)])
    csr = oracle.csr_from_lists(g.variable_lookup, g.check_lookup, g.n, g.m, 3, 6)
    _, ohard, _ = oracle.bp_decode_batch(csr, llr[pick].cpu().numpy(), 50, 0)
    agree = np.all(ohard == hard[pick].cpu().numpy(), axis=1)
    assert agree.mean() >= 0.75


# ---------------------------------------------------------------- Monte-Carlo
def _mc_counters(g, channel, p, seed, B, iters, algo=0, alpha=1.0, early_stop=False, X=-1, stop=0, batches=1):
    import torch
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    mc = MonteCarlo(g, channel, p, iters, algo=algo, alpha=alpha, early_stop=early_stop, expurgation=X, seed=seed,
                    batch=B)
    for i in range(batches):
        mc.run_batch(i * B, B, stop)
    torch.cuda.synchronize()
    return mc.counters.cpu().numpy()


def _oracle_bec_counters(g, p, seed, B, iters, X=-1, stop=0):
    words = oracle.channel(oracle.CH_BEC, p, seed, 0, g.n, B)
    _, err, its = oracle.bec_decode_batch(words, iters, g.variable_lookup, g.check_lookup, g.n, g.k, g.dv, g.dc)
    c = np.zeros(4 + iters + 1, np.int64)
    for b in range(B):
        curve = np.insert(err[b], 0, int(np.count_nonzero(words[b] == 2)))
        if curve[-1] > X:
            c[4:] += curve
            c[1] += curve[-1] != 0
            c[2] += curve[-1]
        c[0] += 1
        c[3] += its[b]
        if stop and c[1] >= stop:
            break
    return c


@pytest.mark.parametrize("X", [-1, 3])
def test_mc_bec_counters_exact(torch, X):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(1000, 3, 6, seed=21)
    got = _mc_counters(g, "bec", 0.42, 77, 2048, 50, X=X)
    np.testing.assert_array_equal(got, _oracle_bec_counters(g, 0.42, 77, 2048, 50, X=X))


def test_mc_bec_sequential_stop_rule(torch):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(1000, 3, 6, seed=22)
    got = _mc_counters(g, "bec", 0.44, 5, 4096, 40, stop=200)
    want = _oracle_bec_counters(g, 0.44, 5, 4096, 40, stop=200)
    assert want[1] == 200
    np.testing.assert_array_equal(got, want)


MC_BITS_CASES = [
    (1000, 65536, -1, 0, "bec_mc_bits_kernel<256,2,u32>"),
    (1000, 131072, 3, 0, "bec_mc_bits_kernel<256,4,u32>"),      # expurgation
    (1000, 131072, -1, 2000, "bec_mc_bits_kernel<256,4,u32>"),  # exact stop inside a batch
    (6000, 4096, -1, 0, "bec_mc_bits_kernel<512,1,u32>"),
    (64800, 512, 3, 0, "bec_mc_bits_kernel<1024,1,u8>"),
]


@pytest.mark.parametrize("n,B,X,stop,kernel", MC_BITS_CASES, ids=["-".join(map(str, c[:-1])) for c in MC_BITS_CASES])
def test_mc_bec_bitsliced_shapes_exact(torch, n, B, X, stop, kernel):
    """The bit-sliced BEC Monte-Carlo kernel (32 codewords per word) at every word width and
    workgroup size it uses, against the oracle's message_passing restatement."""
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    assert bec_plans(n, n // 2, [(BEC_MC, B, 50)])[0]["name"] == kernel
    g = TannerGraph.random_regular(n, 3, 6, seed=23)
    got = _mc_counters(g, "bec", 0.43, 9, B, 50, X=X, stop=stop)
    want = _oracle_bec_counters(g, 0.43, 9, B, 50, X=X, stop=stop)
    if stop:
        assert want[1] == stop and want[0] < B
    np.testing.assert_array_equal(got, want)


def _bec_decode_scalar(decoder, g, words, iters, errors=None, chunk=32):
    """Batch decode in chunks of < 64 words: the per-codeword bec_kernel path."""
    sizes = sorted({min(chunk, len(words) - i) for i in range(0, len(words), chunk)})
    assert all(p["kernel"] == "Word" for p in bec_plans(g.n, g.m, [(BEC_DECODE, b, iters) for b in sizes]))
    outs = [decoder.bec_decode(g, words[i:i + chunk], iters,
                               errors=None if errors is None else errors[i:i + chunk])
            for i in range(0, len(words), chunk)]
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(3))


def test_bec_bitsliced_batch_irregular_vs_scalar_kernel(torch):
    """Irregular CSR graph (RSU, variable degrees 2-4, check degrees up to 8): the
    bit-sliced batch decoder == the per-codeword kernel (pinned to the oracle on CSR
    graphs) on perturbed words with caller errors[]."""
    from iib_project_ldpc_codes_amd import decoder, ensembles
    g = ensembles.sample_irregular(ensembles.RSU_DL4, 2000, seed=5)
    words, errin = _perturbed_bec_batch(g.n, 1000, 0.44, 40, seed=77)
    w, err, its = decoder.bec_decode(g, words, 40, errors=errin)
    sw, serr, sits = _bec_decode_scalar(decoder, g, words, 40, errors=errin)
    np.testing.assert_array_equal(w, sw)
    np.testing.assert_array_equal(err, serr)
    np.testing.assert_array_equal(its, sits)


def test_mc_bec_bitsliced_irregular_vs_scalar_kernel(torch):
    """Irregular CSR graph: bit-sliced MC counters == counters built from the per-codeword
    BEC kernel (itself pinned to the oracle by test_bec_irregular_csr_vs_oracle)."""
    from iib_project_ldpc_codes_amd import decoder, ensembles
    g = ensembles.sample_irregular(ensembles.RSU_DL4, 2000, seed=4)
    B, iters, eps = 8192, 60, 0.45
    got = _mc_counters(g, "bec", eps, 31, B, iters)
    words = oracle.channel(oracle.CH_BEC, eps, 31, 0, g.n, B)
    _, err, its = _bec_decode_scalar(decoder, g, words.astype(np.uint8), iters)
    c = np.zeros(4 + iters + 1, np.int64)
    curves = np.concatenate([np.count_nonzero(words == 2, axis=1)[:, None], err], axis=1)
    c[0] = B
    c[1] = np.count_nonzero(curves[:, -1])
    c[2] = curves[:, -1].sum()
    c[3] = its.sum()
    c[4:] = curves.sum(axis=0)
    np.testing.assert_array_equal(got, c)


@pytest.mark.parametrize("kind,early_stop", [("regular", True), ("csr", True), ("csr", False),
                                             ("rsu20000", True), ("rsu20000", False)])
def test_mc_minsum_bsc_exact(torch, kind, early_stop):
    """Fused Monte-Carlo min-sum (channel + decode + per-iteration counts) against counters built
    from the oracle: the (3,6) LDS kernel, the irregular kernel with every message in LDS (the
    same code as CSR), and the irregular kernel with an L2 slab (RSU n = 20000)."""
    from iib_project_ldpc_codes_amd import ensembles
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    if kind == "rsu20000":
        g = ensembles.sample_irregular(ensembles.RSU_DL4, 20000, seed=5)
        csr, B = g.to_csr(), 96
    else:
        g0 = TannerGraph.random_regular(1000, 3, 6, seed=23)
        csr = oracle.csr_from_lists(g0.variable_lookup, g0.check_lookup, g0.n, g0.m, 3, 6)
        g, B = (g0 if kind == "regular" else TannerGraph.from_csr(*csr)), 512
    iters = 20
    got = _mc_counters(g, "bsc", 0.06, 8, B, iters, algo="minsum", alpha=0.75, early_stop=early_stop)
    llr = oracle.channel(oracle.CH_BSC, 0.06, 8, 0, g.n, B)
    # per-iteration curve from the oracle: run 0..iters iterations
    want = np.zeros(4 + iters + 1, np.int64)
    want[0] = B
    want[4] = int((llr < 0).sum())
    for t in range(1, iters + 1):
        _, h, _ = oracle.bp_decode_batch(csr, llr, t, 1, alpha=0.75, early_stop=early_stop)
        want[4 + t] = int(h.sum())
    _, h, its = oracle.bp_decode_batch(csr, llr, iters, 1, alpha=0.75, early_stop=early_stop)
    want[1] = int(h.any(axis=1).sum())
    want[2] = int(h.sum())
    want[3] = int(its.sum())
    np.testing.assert_array_equal(got, want)


def test_mc_generic_kernel_pushed_off_lds_by_max_iters(torch):
    """(5,10) n = 5,500: the messages fit LDS beside a 500-iteration Monte-Carlo curve but not
    beside a 600-iteration one, so the max_iters = 600 call runs bp_generic_kernel<16,gmem> on
    per-workgroup slabs (once refused: the scratch buffer was sized by a rule that left this call
    out).  Counters against the oracle; the curve against the LDS form of the same kernel."""
    from tests.graph_util import bp_plans, csr_from_checks, regular_simple
    g = regular_simple(5500, 5, 10, seed=1)
    B = 32
    pcsr = csr_from_checks(np.arange(g.m + 1) * 10, g.check_lookup, g.n)
    names = [p["name"] for p in bp_plans(pcsr, [(1, 1, 1, 0, 600, B), (1, 1, 1, 0, 500, B)])]
    assert names == ["bp_generic_kernel<16,gmem>", "bp_generic_kernel<16,lds>"]
    got = _mc_counters(g, "bsc", 0.02, 8, B, 600, algo="minsum", alpha=0.75, early_stop=True)
    csr = oracle.csr_from_lists(g.variable_lookup, g.check_lookup, g.n, g.m, 5, 10)
    llr = oracle.channel(oracle.CH_BSC, 0.02, 8, 0, g.n, B)
    _, h, its = oracle.bp_decode_batch(csr, llr, 600, 1, 0.75, True)
    want = [B, int(h.any(axis=1).sum()), int(h.sum()), int(its.sum())]
    print("counters 0-3: got", got[:4].tolist(), "oracle", want)
    np.testing.assert_array_equal(got[:4], want)
    lds = _mc_counters(g, "bsc", 0.02, 8, B, 500, algo="minsum", alpha=0.75, early_stop=True)
    np.testing.assert_array_equal(got[4:4 + 501], lds[4:4 + 501])


def test_parallel_simulator_fixed_code_device_engine(torch, tmp_path, monkeypatch):
    """run_simulation_fixed_ldpc (parallel_simulator.py:274-401 surface) on the device engine ==
    the oracle's sequential loop over the same Philox trials, including the 200-frame stop."""
    from iib_project_ldpc_codes_amd import parallel_simulator as ps
    monkeypatch.setattr(ps, "base_directory", str(tmp_path) + "/")
    params = dict(BEC=0.42, num_tests=3000, iterations=30, n=500, dv=3, dc=6, filenumber=1, optimal=False,
                  message_passing=True, batch=256)
    res = ps.run_simulation_fixed_ldpc(params)
    g = ps.load_or_create_fixed_code(1, 500, 3, 6)
    want = _oracle_bec_counters(g, 0.42, 1, 3000, 30, stop=200)
    assert res["num_tests"] == want[0] and res["frame_errors"] == want[1] == 200
    assert res["bit_errors"] == want[2]
    np.testing.assert_allclose(res["error_curve"], want[4:] / (500 * want[0]))
    rows = open(tmp_path / "report_data" / "simulation_data" / res["filename"]).read().splitlines()
    assert len(rows) == 30 + 1 + 2 and rows[-2].startswith("Message passing block-wise error")


def test_parallel_simulator_per_trial_engine(torch, tmp_path, monkeypatch):
    """The reference's own loop (numpy channel, one drop-in call per trial) runs end to end."""
    from iib_project_ldpc_codes_amd import parallel_simulator as ps
    monkeypatch.setattr(ps, "base_directory", str(tmp_path) + "/")
    res = ps.run_simulation_fixed_ldpc(dict(BEC=0.3, num_tests=50, iterations=20, n=200, dv=3, dc=6, filenumber=2,
                                            optimal=False, message_passing=True, engine="per_trial"))
    assert res["num_tests"] == 50 and res["error_curve"][0] == pytest.approx(0.3, abs=0.05)


# ------------------------------------------------------------ random graphs
@pytest.mark.parametrize("n,dv,dc", [(1000, 3, 6), (90, 2, 3), (96, 4, 8), (10000, 3, 6), (30000, 3, 6), (64800, 3, 6)])
def test_device_sampler_matches_oracle(torch, n, dv, dc):
    from iib_project_ldpc_codes_amd import _native
    L = _native.lib()
    G, E = 6, n * dv
    chk = np.zeros(G * E, np.int32)
    var = np.zeros(G * E, np.int32)
    att = np.zeros(G, np.int32)
    rc = L.ldpc_sample_regular(n, dv, dc, 31, 1000, G, chk.ctypes.data, var.ctypes.data, att.ctypes.data)
    assert rc == 0
    for g in range(G):
        ochk, ovar, oatt = oracle.sample_regular(n, dv, dc, 31, 1000 + g)
        assert att[g] == oatt > 0
        np.testing.assert_array_equal(chk[g * E:(g + 1) * E], ochk)
        np.testing.assert_array_equal(var[g * E:(g + 1) * E], ovar)


@pytest.mark.parametrize("n", [2000, 20000, 30000])
def test_device_irregular_sampler_matches_oracle(torch, n):
    """ldpc_sample_csr (RSU rate-1/2 degree structure) == oracle_sample_csr, bit for bit.  By
    the launch plan (ldpc_debug_sample_plan): n = 2000 (E = 5,723) runs the one-level sampler with
    the permutation in LDS, sample_regular_kernel<256,u16,lds>; n = 20000 (E = 57,238) and 30000
    (E = 85,857) run the sequential sampler, sample_seq_kernel<csr,u16> behind its search pass,
    with 4-bit occurrence counters and sample_var_side_kernel<1024,u16> (slot ids below 65,536)
    or <1024,int32>.  The one-level kernels on 512 and 1024 buckets are held by
    tests/test_gpu_sampler_shapes.py."""
    from iib_project_ldpc_codes_amd import _native, ensembles
    vptr, cptr = ensembles.degree_ptrs(ensembles.RSU_DL4, n)
    E, m, G = int(vptr[-1]), len(cptr) - 1, 4
    cv = np.zeros(G * E, np.int32)
    vs = np.zeros(G * E, np.int32)
    att = np.zeros(G, np.int32)
    rc = _native.lib().ldpc_sample_csr(n, m, vptr.ctypes.data, cptr.ctypes.data, 8, 50, G, cv.ctypes.data,
                                       vs.ctypes.data, att.ctypes.data)
    assert rc == 0
    for g in range(G):
        ocv, ovs, oatt = oracle.sample_csr(vptr, cptr, 8, 50 + g)
        assert att[g] == oatt > 0
        np.testing.assert_array_equal(cv[g * E:(g + 1) * E], ocv)
        np.testing.assert_array_equal(vs[g * E:(g + 1) * E], ovs)
    # a sampled irregular graph decodes like its oracle (min-sum is bit-exact)
    from iib_project_ldpc_codes_amd import decoder
    g = ensembles.sample_irregular_device(ensembles.RSU_DL4, n, seed=8, graph_id=50)
    llr = oracle.channel(oracle.CH_AWGN, 0.8, 3, 0, n, 8)
    _, hard, its = decoder.bp_decode(g, llr, 20, "minsum", alpha=0.75)
    _, ohard, _ = oracle.bp_decode_batch(g.to_csr(), llr, 20, 1, alpha=0.75)
    np.testing.assert_array_equal(hard, ohard)


def test_ensemble_mc_matches_oracle(torch):
    """ldpc_mc_ensemble_batch_dev: trial t = graph t + channel word t, counters exact."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    n, B, iters, eps, seed = 200, 96, 20, 0.40, 17
    mc = MonteCarlo.ensemble(n, 3, 6, "bec", eps, iters, seed=seed, batch=B)
    mc.run_batch(0, B)
    torch.cuda.synchronize()
    got = mc.counters.cpu().numpy()
    want = np.zeros(4 + iters + 1, np.int64)
    words = oracle.channel(oracle.CH_BEC, eps, seed, 0, n, B)
    for b in range(B):
        chk, var, _ = oracle.sample_regular(n, 3, 6, seed, b)
        _, err, it = oracle.message_passing(words[b], iters, var, chk, n, n // 2, 3, 6)
        curve = np.insert(err, 0, int(np.count_nonzero(words[b] == 2)))
        want[4:] += curve
        want[1] += curve[-1] != 0
        want[2] += curve[-1]
        want[0] += 1
        want[3] += it
    np.testing.assert_array_equal(got, want)


def test_parallel_simulator_ensemble_device(torch, tmp_path, monkeypatch):
    from iib_project_ldpc_codes_amd import parallel_simulator_expurgated as pse
    from iib_project_ldpc_codes_amd import parallel_simulator as ps
    monkeypatch.setattr(ps, "base_directory", str(tmp_path) + "/")
    res = pse.run_simulation(dict(BEC=0.45, num_tests=2000, iterations=40, n=600, dv=3, dc=6, seed=3, optimal=False,
                                  message_passing=True, expurgation=2, batch=512))
    assert 0 < res["num_tests"] <= 2000 and res["frame_errors"] <= 200
    assert res["filename"].startswith("regular_code_expurgated=2_BEC=0.45")


# ------------------------------------------------------- irregular (config 4)
@pytest.mark.parametrize("n", [2000, 20000])
def test_irregular_rsu_vs_oracle(torch, n):
    """RSU rate-1/2 irregular ensemble: min-sum bit-exact, SPA to tolerance (n=20000 runs the
    global-scratch kernel: 57k edges do not fit one CU's LDS in fp32)."""
    from iib_project_ldpc_codes_amd import decoder, ensembles
    g = ensembles.sample_irregular(ensembles.RSU_DL4, n, seed=5)
    B = 8
    llr = oracle.channel(oracle.CH_AWGN, 0.85, 6, 0, n, B)
    post, hard, its = decoder.bp_decode(g, llr, 20, "minsum", alpha=0.8, early_stop=True)
    opost, ohard, oits = oracle.bp_decode_batch(g.csr, llr, 20, 1, alpha=0.8, early_stop=True)
    np.testing.assert_array_equal(post, opost)
    np.testing.assert_array_equal(its, oits)
    post, hard, its = decoder.bp_decode(g, llr, 3, "spa")
    opost, _, _ = oracle.bp_decode_batch(g.csr, llr, 3, 0)
    np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL)


# ------------------------------------------------------- statistical pins
def test_fixed_code_bec_fer_ber_match_reference_probe(torch, golden):
    """the reference C on a fixed (3,6) n=1000 code, eps=0.4, 50 iterations,
    200k trials gave FER 9.05e-2 and BER 2.13e-2 (= tools/plotting.py:69's 0.0214).  Here:
    the reference-generated n=1000 code of the golden fixtures, 262,144 device trials.
    Tolerance: sampling error of both runs (sigma_FER ~ 9e-4) plus the code-to-code
    spread of fixed-code FER at n=1000 (0.0895 - 0.0914 over 7 codes)."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    g = _graph(golden, 3)
    assert g.n == 1000
    mc = MonteCarlo(g, "bec", 0.4, 50, seed=3, batch=65536)
    for r in range(4):
        mc.run_batch(r * 65536, 65536)
    res = mc.results()
    assert res["num_tests"] == 262144
    assert abs(res["fer"] - 0.0905) < 0.003, res["fer"]
    assert abs(res["ber"] - 0.0213) < 0.0007, res["ber"]


def test_soft_waterfalls_bracket_textbook_bp_thresholds(torch):
    """(3,6) BP thresholds (Richardson-Urbanke): BI-AWGN sigma* = 0.8809, BSC p* = 0.084.
    At n = 10^4 with 50 sum-product iterations, 4096 frames: well below the threshold
    almost every frame decodes, well above almost none does."""
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(10000, 3, 6, seed=1, distinct_columns=True)

    def fer(ch, p):
        llr = decoder.channel_dev(ch, p, 21, 0, g.n, 4096)
        _, hard, _ = decoder.bp_decode_dev(g, llr, 50, "spa", early_stop=True, want_post=False)
        return float(hard.any(dim=1).float().mean().item())

    assert fer("awgn", 0.80) < 0.01 and fer("awgn", 0.95) > 0.99
    assert fer("bsc", 0.070) < 0.01 and fer("bsc", 0.100) > 0.99
