"""bp_loc_chain_kernel, the kernel of the chained layout (csrc/bp_loc_chain.hpp; csrc/loc_layout.cpp, build_loc_chain_layout): fixed-count
sum-product decodes of (3,6) codes at the 512 x 5 shape, n = 4,100 (the smallest: a part-filled
wave and idle waves) and n = 10,000 (the bench shape), against the oracle and against the same
decodes on the plain layout (LDPC_NO_LOC_CHAIN=1, a fresh graph handle).  Tolerances are
tests/test_gpu_loc.py's.  Min-sum and early-stop decodes must not take the chained path: their
results are bit-identical with and without it."""
import functools

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

SPA_RTOL, SPA_ATOL = 1e-4, 1e-4
SIZES = [4100, 10000]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


def _graph(n, chain, monkeypatch):
    """A fresh handle whose layouts are built with or without the chained one."""
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    monkeypatch.delenv("LDPC_NO_LOC_LAYOUT", raising=False)
    monkeypatch.delenv("LDPC_LOC_T", raising=False)
    if chain:
        monkeypatch.delenv("LDPC_NO_LOC_CHAIN", raising=False)
    else:
        monkeypatch.setenv("LDPC_NO_LOC_CHAIN", "1")
    g = TannerGraph.random_regular(n, 3, 6, seed=21)
    g.handle()  # the layouts are built now, under this environment
    assert g.kernel_name() == "bp_loc_kernel"
    return g


@functools.lru_cache(maxsize=None)
def _csr(n):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    return tuple(np.ascontiguousarray(a, np.int32) for a in TannerGraph.random_regular(n, 3, 6, seed=21).to_csr())


@functools.lru_cache(maxsize=None)
def _oracle_spa(n, iters, sigma, seed, B):
    llr = oracle.channel(oracle.CH_AWGN, sigma, seed, 0, n, B)
    return (llr,) + tuple(oracle.bp_decode_batch(list(_csr(n)), llr, iters, 0))


@pytest.mark.parametrize("n", SIZES)
def test_chain_spa_vs_oracle_and_plain(torch, monkeypatch, n):
    from iib_project_ldpc_codes_amd import decoder
    g = _graph(n, True, monkeypatch)
    plain = _graph(n, False, monkeypatch)
    for iters in (1, 3, 5):
        llr, opost, ohard, _ = _oracle_spa(n, iters, 0.82, 5, 32)
        post, hard, its = decoder.bp_decode(g, llr, iters, "spa")
        np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL)
        assert np.all(its == iters)
        ppost, phard, pits = decoder.bp_decode(plain, llr, iters, "spa")
        np.testing.assert_allclose(post, ppost, rtol=SPA_RTOL, atol=SPA_ATOL)
        assert np.array_equal(its, pits)
        # the two layouts multiply a variable's ratios in different orders: equal to the last
        # bit everywhere would mean the chained path did not run
        assert not np.array_equal(post, ppost)


@pytest.mark.parametrize("n", SIZES)
def test_chain_spa_50_iterations(torch, monkeypatch, n):
    """test_loc_spa_50_iterations' criterion, against the oracle and against the plain layout."""
    from iib_project_ldpc_codes_amd import decoder
    llr, opost, ohard, _ = _oracle_spa(n, 50, 0.85, 7, 64)
    post, hard, its = decoder.bp_decode(_graph(n, True, monkeypatch), llr, 50, "spa")
    ppost, phard, pits = decoder.bp_decode(_graph(n, False, monkeypatch), llr, 50, "spa")
    for ref_post, ref_hard in ((opost, ohard), (ppost.astype(np.float64), phard)):
        same = np.all(hard == ref_hard, axis=1)
        assert same.mean() >= 0.99
        d = np.abs(post[same].astype(np.float64) - ref_post[same])
        assert np.mean(d <= 1e-3 + 1e-3 * np.abs(ref_post[same])) >= 0.999
    assert np.array_equal(its, pits)


@pytest.mark.parametrize("n", SIZES)
def test_other_modes_keep_the_plain_layout(torch, monkeypatch, n):
    from iib_project_ldpc_codes_amd import decoder
    g = _graph(n, True, monkeypatch)
    plain = _graph(n, False, monkeypatch)
    llr = oracle.channel(oracle.CH_AWGN, 0.82, 6, 0, n, 32)
    for algo, early_stop in (("minsum", False), ("minsum", True), ("spa", True)):
        got = decoder.bp_decode(g, llr, 20, algo, alpha=0.75, early_stop=early_stop)
        want = decoder.bp_decode(plain, llr, 20, algo, alpha=0.75, early_stop=early_stop)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
