"""bp_loc_kernel (local-edge layout, csrc/loc_layout.cpp) against the oracle, and the same
decodes with the layout disabled (LDPC_NO_LOC_LAYOUT=1 -> bp_lds_kernel / bp_irr_kernel /
bp_generic_kernel) so both paths stay covered.  Shapes: (3,6) n = 1,000 (256 threads, one
check pair each), n = 10,000 (the bench code: 1024 threads, 2-3 pairs), RSU rate-1/2
irregular n = 2,000 and 20,000 (absent edges, two check-degree classes), with the zigzag
and the ring (configs[3]'s code, ensembles.py deg2="path") degree-2 placements.  Tolerances as in
test_gpu_parity.py: min-sum bit-exact; sum-product posteriors within SPA_* after 1-5
iterations."""
import functools

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

SPA_RTOL, SPA_ATOL = 1e-4, 1e-4


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


@functools.lru_cache(maxsize=None)
def _rsu_csr(n, seed, deg2):
    from iib_project_ldpc_codes_amd import ensembles
    return tuple(np.asarray(a) for a in ensembles.sample_irregular(ensembles.RSU_DL4, n, seed=seed, deg2=deg2).to_csr())


def _graph(kind, n, seed, noloc, monkeypatch):
    from iib_project_ldpc_codes_amd import ensembles
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    if noloc:
        monkeypatch.setenv("LDPC_NO_LOC_LAYOUT", "1")
    else:
        monkeypatch.delenv("LDPC_NO_LOC_LAYOUT", raising=False)
    if kind in ("rsu", "ring"):
        g = TannerGraph.from_csr(*_rsu_csr(n, seed, "zigzag" if kind == "rsu" else "path"))
    else:
        g = TannerGraph.random_regular(n, 3, 6, seed=seed)
    g.handle()  # the layout is built (or not) now, under this environment
    return g, [np.ascontiguousarray(a, np.int32) for a in g.to_csr()]


CASES = [("reg", 1000), ("reg", 10000), ("rsu", 2000), ("rsu", 20000), ("ring", 20000)]


@pytest.mark.parametrize("kind,n", CASES)
@pytest.mark.parametrize("noloc", [False, True])
def test_loc_spa_vs_oracle(torch, monkeypatch, kind, n, noloc):
    from iib_project_ldpc_codes_amd import decoder
    g, csr = _graph(kind, n, 21 if kind != "ring" else 1, noloc, monkeypatch)
    assert (g.kernel_name() == "bp_loc_kernel") != noloc
    llr = oracle.channel(oracle.CH_AWGN, 0.82, 5, 0, g.n, 32)
    for iters in (1, 3, 5):
        post, hard, its = decoder.bp_decode(g, llr, iters, "spa")
        opost, ohard, _ = oracle.bp_decode_batch(csr, llr, iters, 0)
        np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL)
        assert np.all(its == iters)


@pytest.mark.parametrize("kind,n", CASES)
def test_loc_minsum_bit_exact(torch, monkeypatch, kind, n):
    """Min-sum through the local kernel's ordered variable sums (the (3,6) n = 1,000 code:
    256-thread shape; n = 10,000: the two-workgroup 512-thread shape) -- bit-exact."""
    from iib_project_ldpc_codes_amd import decoder
    g, csr = _graph(kind, n, 22 if kind != "ring" else 1, False, monkeypatch)
    llr = oracle.channel(oracle.CH_AWGN, 0.80, 6, 0, g.n, 32)
    post, hard, its = decoder.bp_decode(g, llr, 20, "minsum", alpha=0.75)
    opost, ohard, oits = oracle.bp_decode_batch(csr, llr, 20, 1, alpha=0.75)
    np.testing.assert_array_equal(post, opost)
    np.testing.assert_array_equal(hard, ohard)


def _plan(csr, algo, env=None):
    """Kernel name and threads of a 2-word, 5-iteration decode with posteriors (host-only plan)."""
    from tests.graph_util import bp_plans
    p = bp_plans(csr, [(algo, 0, 0, 1, 5, 2)], env=env)[0]
    return p["name"], p["threads"]


# Every row of the bp_lds_kernel<3,6> shape table (csrc/kernel_shapes.hpp) that a graph can reach (no n
# reaches 1024 x 2), each at the smallest even n whose lane layout has that (threads, variables per
# thread): just above threads x the row before / 1.02 (256 x 1: n = 96).
LDS36_ROWS = [(96, 256, 1), (252, 256, 2), (502, 256, 3), (754, 256, 5), (1256, 256, 9), (2050, 1024, 3),
              (3012, 1024, 5), (5020, 1024, 6), (6024, 1024, 9), (9036, 1024, 10), (10040, 1024, 11), (11044, 1024, 14)]


@pytest.mark.parametrize("n,T,VPT", LDS36_ROWS)
def test_lds36_every_shape(torch, monkeypatch, n, T, VPT):
    """Min-sum on bp_lds_kernel<3,6> (the local-edge layout disabled), two words, five iterations:
    bit-exact against the oracle at every (threads, variables per thread) of the table."""
    from iib_project_ldpc_codes_amd import decoder
    from tests.test_host_layouts import lane_layout
    g, csr = _graph("reg", n, 21, True, monkeypatch)
    lane = lane_layout((np.ascontiguousarray(g.variable_lookup, np.int32), np.ascontiguousarray(g.check_lookup, np.int32),
                        n, n // 2, 3, 6))
    assert (lane["T"], lane["VPT"]) == (T, VPT)
    assert _plan(csr, 1, {"LDPC_NO_LOC_LAYOUT": "1"}) == ("bp_lds_kernel<3,6>", T)
    assert g.kernel_name() == "bp_lds_kernel<3,6>"
    llr = oracle.channel(oracle.CH_AWGN, 0.80, 6, 0, n, 2)
    post, hard, its = decoder.bp_decode(g, llr, 5, "minsum", alpha=0.75)
    opost, ohard, _ = oracle.bp_decode_batch(csr, llr, 5, 1, alpha=0.75)
    np.testing.assert_array_equal(post, opost)
    np.testing.assert_array_equal(hard, ohard)


# The (3,6) rows of the bp_loc_kernel shape table that no other test launches, at the smallest n of
# whole check pairs with that (threads, check pairs per thread): n / 4 = 256 (pairs - 1) + 1 pairs on
# 256 threads, and 2,561 pairs, the first past the 512 x 5 shape, on 1,024.  (256 x 1 and 512 x 5 run
# at n = 1,000 and 10,000 above; a (3,6) code never gets 1024 x 2: up to 2,560 pairs it takes 512
# threads.)
LOC36_ROWS = [(1028, 256, 2), (2052, 256, 3), (3076, 256, 4), (10244, 1024, 3)]


@pytest.mark.parametrize("n,T,KP", LOC36_ROWS)
def test_loc_reg36_every_shape(torch, monkeypatch, n, T, KP):
    """Sum-product on bp_loc_kernel (min-sum runs on bp_lds_kernel<3,6> at these shapes), two words,
    1, 3 and 5 iterations: posteriors within SPA_* of the oracle, as test_loc_spa_vs_oracle."""
    from iib_project_ldpc_codes_amd import decoder
    from tests.test_host_layouts import loc_layout, loc_variant
    g, csr = _graph("reg", n, 21, False, monkeypatch)
    assert _plan(csr, 0) == ("bp_loc_kernel", T)
    assert loc_layout(csr, T)["shape"][:2] == [T, KP] and loc_variant(csr, T)["variant"] == 1
    assert g.kernel_name() == "bp_loc_kernel"
    llr = oracle.channel(oracle.CH_AWGN, 0.82, 5, 0, n, 2)
    for iters in (1, 3, 5):
        post, hard, its = decoder.bp_decode(g, llr, iters, "spa")
        opost, ohard, _ = oracle.bp_decode_batch(csr, llr, iters, 0)
        np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL)
        assert np.all(its == iters)


# The RSU-variant rows of the table that no case above launches (256 x 2 and 512 x 10 run at n = 2,000
# and 20,000), at the smallest n of whole check pairs with that shape: 256 threads up to 1,024 pairs
# (n / 4 = 256 (pairs - 1) + 1; 256 x 1: n = 500), 1,024 up to 3,072, 512 beyond.
LOC_RSU_ROWS = [(500, 256, 1), (2052, 256, 3), (3076, 256, 4), (4100, 1024, 2), (8196, 1024, 3), (12292, 512, 8)]


@pytest.mark.parametrize("n,T,KP", LOC_RSU_ROWS)
def test_loc_rsu_every_shape(torch, monkeypatch, n, T, KP):
    """Min-sum on bp_loc_kernel's RSU instantiation, two words, five iterations: bit-exact against
    the oracle, as test_loc_minsum_bit_exact."""
    from iib_project_ldpc_codes_amd import decoder
    from tests.test_host_layouts import loc_layout, loc_variant
    g, csr = _graph("rsu", n, 21, False, monkeypatch)
    assert _plan(csr, 1) == ("bp_loc_kernel", T)
    assert loc_layout(csr, T)["shape"][:2] == [T, KP] and loc_variant(csr, T)["variant"] == 2
    assert g.kernel_name() == "bp_loc_kernel"
    llr = oracle.channel(oracle.CH_AWGN, 0.80, 6, 0, g.n, 2)
    post, hard, its = decoder.bp_decode(g, llr, 5, "minsum", alpha=0.75)
    opost, ohard, _ = oracle.bp_decode_batch(csr, llr, 5, 1, alpha=0.75)
    np.testing.assert_array_equal(post, opost)
    np.testing.assert_array_equal(hard, ohard)


@pytest.mark.parametrize("kind,n", [("reg", 10000), ("rsu", 20000)])
def test_loc_spa_50_iterations(torch, monkeypatch, kind, n):
    """50 iterations: identical hard decisions on >= 99 % of frames and posteriors of those
    frames within 1e-3 abs + 1e-3 rel for >= 99.9 % of values (the kernel's fp32 product
    form against the oracle's double-precision check rule)."""
    from iib_project_ldpc_codes_amd import decoder
    g, csr = _graph(kind, n, 23, False, monkeypatch)
    llr = oracle.channel(oracle.CH_AWGN, 0.80 if kind == "rsu" else 0.85, 7, 0, g.n, 64)
    post, hard, _ = decoder.bp_decode(g, llr, 50, "spa")
    opost, ohard, _ = oracle.bp_decode_batch(csr, llr, 50, 0)
    same = np.all(hard == ohard, axis=1)
    assert same.mean() >= 0.99
    d = np.abs(post[same].astype(np.float64) - opost[same])
    assert np.mean(d <= 1e-3 + 1e-3 * np.abs(opost[same])) >= 0.999


@pytest.mark.parametrize("kind,n,sigma", [("reg", 10000, 0.86), ("rsu", 20000, 0.84), ("ring", 20000, 0.88)])
@pytest.mark.parametrize("early_stop", [True, False])
def test_loc_mc_spa_vs_oracle(torch, monkeypatch, kind, n, sigma, early_stop):
    """Fused Monte-Carlo sum-product on bp_loc_kernel (Philox channel, sign-bit syndrome early
    stop): counters against the oracle's decodes of the same channel frames.  Sum-product is
    compared to tolerance (the kernel's fp32 rule vs the oracle's exact one): frame errors
    within 2, bit errors within 2 % + 20, iteration totals within 0.5 %."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    g, csr = _graph(kind, n, 24 if kind != "ring" else 1, False, monkeypatch)
    assert g.kernel_name() == "bp_loc_kernel"
    B, iters = 128, 30
    mc = MonteCarlo(g, "awgn", sigma, iters, algo="spa", early_stop=early_stop, seed=31, batch=B)
    mc.run_batch(0, B)
    torch.cuda.synchronize()
    got = mc.counters.cpu().numpy()
    llr = oracle.channel(oracle.CH_AWGN, sigma, 31, 0, g.n, B)
    _, h, its = oracle.bp_decode_batch(csr, llr, iters, 0, early_stop=early_stop)
    fe, be = int(h.any(axis=1).sum()), int(h.sum())
    assert got[0] == B
    assert 0 < fe < B  # both decoded and failed frames at this sigma
    assert abs(int(got[1]) - fe) <= 2, (got[:4], fe, be, int(its.sum()))
    assert abs(int(got[2]) - be) <= 0.02 * be + 20, (got[:4], fe, be)
    assert abs(int(got[3]) - int(its.sum())) <= 0.005 * its.sum() + 2, (got[:4], int(its.sum()))
    assert got[4] == int((llr < 0).sum())  # channel errors: bit-exact (Philox + fused channel)
    assert got[4 + iters] == got[2]  # the last curve point is the final error count


@pytest.mark.parametrize("kind,n", [("reg", 1000), ("reg", 10000)])
@pytest.mark.parametrize("early_stop", [True, False])
def test_loc_mc_minsum_exact(torch, monkeypatch, kind, n, early_stop):
    """Fused Monte-Carlo min-sum on bp_loc_kernel (configs[2]: BSC, normalized min-sum), with the
    LDS-syndrome early stop (decision changes XOR their checks' syndrome bits): every counter
    -- frames, frame / bit errors, iterations, the per-iteration error curve -- bit-exact
    against the oracle's decodes of the same Philox channel frames."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    g, csr = _graph(kind, n, 25, False, monkeypatch)
    assert g.kernel_name() == "bp_loc_kernel"
    B, iters, p = 192, 20, (0.065 if n == 1000 else 0.076)  # failing frames at both lengths
    mc = MonteCarlo(g, "bsc", p, iters, algo="minsum", alpha=0.75, early_stop=early_stop, seed=8, batch=B)
    mc.run_batch(0, B)
    torch.cuda.synchronize()
    got = mc.counters.cpu().numpy()
    llr = oracle.channel(oracle.CH_BSC, p, 8, 0, g.n, B)
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
    assert 0 < want[1] < B  # both decoded and failed frames at this crossover probability
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("m", [1000, 10000])
def test_loc_check6_var24_vs_oracle(torch, monkeypatch, m):
    """Advisor round 2 (high): a check-regular degree-6 graph with variable degrees {2, 4}
    has loc_dlo == 6 but DVN = 3; it must run on the RSU instantiation (its DVN = 3 gather
    rows and absent-edge flags), not the (3,6) one.  SPA posteriors within tolerance and
    min-sum bit-exact against the oracle, at the 256-thread (m = 1,000) and 512-thread
    (m = 10,000) shapes; and the Monte-Carlo sum-product counters with early stop."""
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    from tests.graph_util import check6_var24
    monkeypatch.delenv("LDPC_NO_LOC_LAYOUT", raising=False)
    g = check6_var24(m, seed=5)
    csr = [np.ascontiguousarray(a, np.int32) for a in g.to_csr()]
    assert g.kernel_name() == "bp_loc_kernel"
    llr = oracle.channel(oracle.CH_AWGN, 0.80, 5, 0, g.n, 32)
    for iters in (1, 3, 5):
        post, hard, its = decoder.bp_decode(g, llr, iters, "spa")
        opost, ohard, _ = oracle.bp_decode_batch(csr, llr, iters, 0)
        np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL)
    post, hard, its = decoder.bp_decode(g, llr, 20, "minsum", alpha=0.75)
    opost, ohard, _ = oracle.bp_decode_batch(csr, llr, 20, 1, alpha=0.75)
    np.testing.assert_array_equal(post, opost)
    np.testing.assert_array_equal(hard, ohard)
    B, iters = 128, 20
    mc = MonteCarlo(g, "awgn", 0.80, iters, algo="spa", early_stop=True, seed=3, batch=B)
    mc.run_batch(0, B)
    torch.cuda.synchronize()
    got = mc.counters.cpu().numpy()
    llr = oracle.channel(oracle.CH_AWGN, 0.80, 3, 0, g.n, B)
    _, h, its = oracle.bp_decode_batch(csr, llr, iters, 0, early_stop=True)
    fe, be = int(h.any(axis=1).sum()), int(h.sum())
    assert got[0] == B and got[4] == int((llr < 0).sum())
    assert abs(int(got[1]) - fe) <= 2, (got[:4], fe, be)
    assert abs(int(got[3]) - int(its.sum())) <= 0.005 * its.sum() + 2, (got[:4], int(its.sum()))
