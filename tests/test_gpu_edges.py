"""Edge cases of the HIP path through the C ABI, against the oracle / the reference's semantics.

* Empty batches (B = 0) on every device entry point: LDPC_OK, nothing written.
* Zero iterations: message_passing returns 0 and leaves Mvc and errors alone (message_passing.c:14,
  the loop body never runs); the batched BEC decode leaves the words alone with its = 0; the soft
  decoders return the channel LLRs as posteriors (oracle_bp_decode, ldpc_oracle.c, max_iters == 0):
  min-sum bit-exact, sum-product within 1e-6 relative (the LLR makes the round trip through the
  kernels' log2 message domain), hard decisions identical.
* Degenerate BEC words: all erased (stall from iteration 2 on, message_passing.c:16-19), no
  erasure (converged at iteration 0), a single erasure, known ones (non-codeword data), on the
  per-codeword kernel (B < 64) and the bit-sliced one (B >= 64) -- bit-exact with the oracle.
* Channel values the reference never rejects but a GPU kernel can mishandle: Mvc outside {0,1,2}
  is refused with LDPC_EINVAL (the C ABI's error convention) instead of decoding garbage.
* Soft inputs at the edges of fp32: LLR = 0 and -0 (erasure-like), 1e-30, 1e4, 1e30 (beyond the
  kernels' 87-nat staging clamp, re-read from the input for the posterior), on every soft kernel
  (bp_loc_kernel, bp_lds_kernel, bp_irr_kernel, bp_generic_kernel via LDPC_NO_LOC_LAYOUT and
  early stop): min-sum bit-exact; sum-product hard decisions identical and posteriors within
  SAT_ATOL + SAT_RTOL |post| (test_gpu_parity.py's saturated-message tolerance) after 1-3
  iterations.
"""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests.graph_util import extreme_llrs

pytestmark = pytest.mark.gpu

SAT_ATOL, SAT_RTOL = 1e-3, 3e-3


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


@pytest.fixture(scope="module")
def lib():
    from iib_project_ldpc_codes_amd import _native
    return _native.lib()


@functools.lru_cache(maxsize=None)
def _rsu_csr(n, seed):
    from iib_project_ldpc_codes_amd import ensembles
    return tuple(np.asarray(a) for a in ensembles.sample_irregular(ensembles.RSU_DL4, n, seed=seed).to_csr())


def _graph(kind, n, noloc, monkeypatch):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    if noloc:
        monkeypatch.setenv("LDPC_NO_LOC_LAYOUT", "1")
    else:
        monkeypatch.delenv("LDPC_NO_LOC_LAYOUT", raising=False)
    g = TannerGraph.from_csr(*_rsu_csr(n, 31)) if kind == "rsu" else TannerGraph.random_regular(n, 3, 6, seed=31)
    g.handle()
    return g, [np.ascontiguousarray(a, np.int32) for a in g.to_csr()]


SOFT = [("reg", 1000, False), ("reg", 10000, False), ("reg", 10000, True), ("rsu", 2000, False),
        ("rsu", 2000, True)]


# ------------------------------------------------------------------ empty / zero
def test_empty_batches(torch, lib):
    from iib_project_ldpc_codes_amd import _native, decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(1000, 3, 6, seed=3)
    words = torch.empty((0, g.n), dtype=torch.uint8, device="cuda")
    _, err, its = decoder.bec_decode_dev(g, words, 50)
    assert err.shape == (0, 50) and its.shape == (0,)
    llr = torch.empty((0, g.n), dtype=torch.float32, device="cuda")
    for algo in ("spa", "minsum"):
        for es in (False, True):
            post, hard, its = decoder.bp_decode_dev(g, llr, 10, algo, 0.75, es)
            assert post.shape == (0, g.n) and its.shape == (0,)
    out, uns = decoder.ml_decode_dev(g, words)
    assert out.shape == (0, g.n)
    torch.cuda.synchronize()
    assert _native.LDPC_OK == 0


def test_dropin_zero_iterations_and_bad_values(lib):
    from iib_project_ldpc_codes_amd import _native
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(200, 3, 6, seed=4)
    v2c = np.ascontiguousarray(g.variable_lookup, np.int32)
    c2v = np.ascontiguousarray(g.check_lookup, np.int32)
    word = np.where(np.random.RandomState(0).rand(g.n) < 0.4, 2, 0).astype(np.int32)
    keep = word.copy()
    errors = np.arange(5, dtype=np.int32)
    it = lib.message_passing(word.ctypes.data, 0, v2c.ctypes.data, c2v.ctypes.data, errors.ctypes.data,
                             g.n, g.k, 3, 6)
    assert it == 0
    np.testing.assert_array_equal(word, keep)
    np.testing.assert_array_equal(errors, np.arange(5))
    bad = keep.copy()
    bad[7] = 3
    errors = np.zeros(20, np.int32)
    rc = lib.message_passing(bad.ctypes.data, 20, v2c.ctypes.data, c2v.ctypes.data, errors.ctypes.data,
                             g.n, g.k, 3, 6)
    assert rc == _native.LDPC_EINVAL
    assert np.all(errors == 0)
    # the library still decodes after a refused call
    ow, oerr, oit = oracle.message_passing(keep, 20, v2c, c2v, g.n, g.k, 3, 6)
    errors = np.zeros(20, np.int32)
    it = lib.message_passing(keep.ctypes.data, 20, v2c.ctypes.data, c2v.ctypes.data, errors.ctypes.data,
                             g.n, g.k, 3, 6)
    assert it == oit
    np.testing.assert_array_equal(keep, ow)
    np.testing.assert_array_equal(errors, oerr)


@pytest.mark.parametrize("B", [8, 128])
def test_bec_zero_iterations(torch, B):
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(1000, 3, 6, seed=5)
    words = oracle.channel(oracle.CH_BEC, 0.4, 8, 0, g.n, B).astype(np.uint8)
    w, err, its = decoder.bec_decode(g, words, 0)
    np.testing.assert_array_equal(w, words)
    assert err.shape == (B, 0) and np.all(its == 0)


@pytest.mark.parametrize("B", [8, 128])
def test_bec_degenerate_words_vs_oracle(torch, B):
    """All erased / none erased / one erasure / known ones, bit-exact with the oracle."""
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(1000, 3, 6, seed=6)
    rs = np.random.RandomState(B)
    words = np.zeros((B, g.n), np.uint8)
    words[0::4] = 2                                   # all erased: stalls at the first iteration
    words[2::4, rs.randint(g.n)] = 2                  # a single erasure
    ones = np.where(rs.rand(B // 4, g.n) < 0.3, 2, np.where(rs.rand(B // 4, g.n) < 0.05, 1, 0))
    words[3::4] = ones                                # erasures + known ones (not a codeword)
    for iters in (1, 2, 3, 50):
        w, err, its = decoder.bec_decode(g, words, iters)
        ow, oerr, oits = oracle.bec_decode_batch(words, iters, g.variable_lookup, g.check_lookup, g.n, g.k, 3, 6)
        np.testing.assert_array_equal(w.astype(np.int8), ow)
        np.testing.assert_array_equal(err, oerr)
        np.testing.assert_array_equal(its, oits)
    assert np.all(err[0::4] == g.n) and np.all(its[1::4] == 0)


# ------------------------------------------------------------------------- soft
@pytest.mark.parametrize("kind,n,noloc", SOFT)
@pytest.mark.parametrize("algo", ["spa", "minsum"])
@pytest.mark.parametrize("early_stop", [False, True])
def test_bp_zero_iterations(torch, monkeypatch, kind, n, noloc, algo, early_stop):
    from iib_project_ldpc_codes_amd import decoder
    g, csr = _graph(kind, n, noloc, monkeypatch)
    llr = oracle.channel(oracle.CH_AWGN, 0.85, 9, 0, g.n, 16)
    llr[:, :5] = 0.0
    llr[:, 5] = -0.0
    post, hard, its = decoder.bp_decode(g, llr, 0, algo, 0.75, early_stop)
    opost, ohard, oits = oracle.bp_decode_batch(csr, llr, 0, 0 if algo == "spa" else 1, 0.75, early_stop)
    if algo == "spa":  # the LLR goes through the kernels' log2 message domain and back: ~1 ulp
        np.testing.assert_allclose(post, opost, rtol=1e-6, atol=1e-6)
    else:
        np.testing.assert_array_equal(post, opost)
    np.testing.assert_array_equal(hard, ohard)
    np.testing.assert_array_equal(its, oits)


@pytest.mark.parametrize("kind,n,noloc", SOFT)
@pytest.mark.parametrize("early_stop", [False, True])
def test_minsum_extreme_llrs_bit_exact(torch, monkeypatch, kind, n, noloc, early_stop):
    from iib_project_ldpc_codes_amd import decoder
    g, csr = _graph(kind, n, noloc, monkeypatch)
    llr = extreme_llrs(g.n, 24, 11)
    for iters in (1, 3, 10):
        post, hard, its = decoder.bp_decode(g, llr, iters, "minsum", 0.75, early_stop)
        opost, ohard, oits = oracle.bp_decode_batch(csr, llr, iters, 1, 0.75, early_stop)
        np.testing.assert_array_equal(hard, ohard)
        np.testing.assert_array_equal(its, oits)
        np.testing.assert_array_equal(post, opost)


@pytest.mark.parametrize("kind,n,noloc", SOFT)
def test_spa_extreme_llrs(torch, monkeypatch, kind, n, noloc):
    from iib_project_ldpc_codes_amd import decoder
    g, csr = _graph(kind, n, noloc, monkeypatch)
    llr = extreme_llrs(g.n, 24, 12)
    for iters in (1, 2, 3):
        post, hard, its = decoder.bp_decode(g, llr, iters, "spa")
        opost, ohard, _ = oracle.bp_decode_batch(csr, llr, iters, 0)
        assert np.all(np.isfinite(post))
        np.testing.assert_allclose(post, opost, rtol=SAT_RTOL, atol=SAT_ATOL)
        # decisions differ only where the oracle's posterior is within the tolerance of 0
        diff = hard != ohard
        assert np.all(np.abs(opost[diff]) <= SAT_ATOL), (iters, int(diff.sum()))
