"""bp_layer_kernel (csrc/bp_layer.hip), the layered (row-serial) schedule on a fixed code, against
the numpy reference of its contract (tests/layered_ref.py: a sequential sweep over the checks
sorted by (layer, check id), the layers from ldpc_debug_layer_schedule).

Every case first holds the launch plan of its own calls (layer_plans) to the kernel name it
claims -- bp_layer_kernel<8|16|32,lds> for blocks P | R that fit LDS, <*,gmem> (0 < lds_slots <
n + E: words really stored in the slab) for the others.

* Min-sum, alpha = 0.75: post / hard / its bit-exact, fixed count and early stop, 1 / 3 / 20
  iterations, on 24 BI-AWGN frames (sigma 0.80, seed 13) and graph_util.extreme_llrs; LDS form:
  (3,6) n = 600, r58_320, r510_640, r324_1024, mixA, mixB; slab form: r58_8800, r432_12288 and the
  headline (3,6) n = 10,000.  (One reference run per graph, frame set and mode: a decode of t
  iterations is a prefix of the 20-iteration one.)
* More codewords than workgroups: B = 264 on the 256-workgroup grid of a slab graph.
* A layer larger than the workgroup, once per form: the smallest (3,6) n whose largest layer
  exceeds the plan's threads by >= 10 % (n = 5,060: 282 checks on 256 threads; n = 20,270: 1,127 on
  1,024; two less and the layer is one check short -- asserted from the schedule and the plan).
* Sum-product, unsaturated (reference posteriors below the 23 ln 2 clamp, asserted): 1 / 3 / 5
  iterations within SPA_ATOL + SPA_RTOL |post|, the project's 1e-4 / 1e-4.
* Sum-product, saturated (a sigma per graph at which the reference decodes every frame and its
  posteriors pass the clamp, both asserted): 3 and 10 iterations, fixed count and early stop,
  finite posteriors within SAT_ATOL + SAT_RTOL |post|, its equal on >= 98 % of frames.
* Fused Monte-Carlo: min-sum on the BSC with every counter and the whole curve bit-exact (one case
  with expurgation and a stop_frame_errors cut inside the batch); sum-product on BI-AWGN within
  tests/test_gpu_fallback.py::test_mc_spa_awgn_vs_oracle's tolerances.
* schedule="flooding" is the call without the argument, bit for bit.
* A layered MonteCarlo run over two batches equals two runs joined by a snapshot.

Each sum-product case dumps its achieved margins (tests/test_gpu_fullsize.py's _dump).
"""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import layered_ref
from tests.graph_util import extreme_llrs
from tests.layered_util import graph, graph_csr, kernel_name, layer_plans, layers, schedule
from tests.test_gpu_fullsize import _dump

pytestmark = pytest.mark.gpu

SPA_ATOL, SPA_RTOL = 1e-4, 1e-4   # tests/test_gpu_parity.py
SAT_ATOL, SAT_RTOL = 1e-3, 3e-3   # tests/test_gpu_edges.py
XMAX = layered_ref.XMAX
B = 24

LDS_GRAPHS = ["r36_600", "r58_320", "r510_640", "r324_1024", "mixA", "mixB"]
SLAB_GRAPHS = ["r58_8800", "r432_12288", "r36_10000"]
# sigma at which max |reference posterior| < XMAX after 1, 3 and 5 iterations of 8 frames of seed 21
# (found on the CPU; tests/test_gpu_fallback.py's UNSAT_SIGMA for its graphs)
UNSAT = [("r36_600", 0.95), ("r510_640", 0.85), ("r324_1024", 0.75), ("mixB", 1.00)]
# sigma at which the reference decodes all 32 frames of seed 3 within 10 iterations and its
# posteriors pass the clamp (found on the CPU)
SATURATED = [("r36_600", 0.6), ("r510_640", 0.6), ("r324_1024", 0.35), ("r58_8800", 0.7)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


def _routed(name, calls, lds):
    """The plans of `calls` (algo, early_stop, mc, want_post, iters, B) on graph `name`, each
    held to the form the case claims."""
    csr = graph_csr(name)
    plans = layer_plans(csr, calls)
    for call, p in zip(calls, plans):
        assert p["name"] == kernel_name(csr, lds), (name, call, p)
        if not lds:
            assert 0 < p["lds_slots"] < csr[2].size - 1 + csr[1].size, (name, call, p)
    return plans


def _decode(name, llr, iters, algo, alpha=1.0, early_stop=False, **kw):
    from iib_project_ldpc_codes_amd import decoder
    return decoder.bp_decode(graph(name), llr, iters, algo, alpha, early_stop, schedule="layered", **kw)


@functools.lru_cache(maxsize=None)
def _awgn(n, sigma, seed, frames):
    return oracle.channel(oracle.CH_AWGN, sigma, seed, 0, n, frames)


def _ref(name, llr, iters, algo, alpha=1.0, early_stop=False, at=()):
    return layered_ref.decode(graph_csr(name), layers(name)[1], llr, iters, algo, alpha, early_stop, at=at)


def _assert_bit_exact(got, want, what):
    post, hard, its = got
    np.testing.assert_array_equal(hard, want[1], err_msg=str(what))
    np.testing.assert_array_equal(its, want[2], err_msg=str(what))
    np.testing.assert_array_equal(post.view(np.uint32), want[0].view(np.uint32), err_msg=str(what))


def _spa_margins(post, rpost):
    d = np.abs(post.astype(np.float64) - rpost)
    ref = np.abs(rpost.astype(np.float64))
    return {"post_max_abs": float(np.nanmax(d)) if np.isfinite(d).any() else None,
            "ref_post_max_abs": float(ref.max()),
            "within_spa_tol_frac": float((d <= SPA_ATOL + SPA_RTOL * ref).mean()),
            "nan_count": int(np.isnan(post).sum())}


# ------------------------------------------------------------------ min-sum
@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("name", LDS_GRAPHS + SLAB_GRAPHS)
def test_minsum_bit_exact(torch, name, early_stop):
    n = graph(name).n
    _routed(name, [(1, int(early_stop), 0, 1, it, B) for it in (1, 3, 20)], name in LDS_GRAPHS)
    for kind, llr in (("awgn", _awgn(n, 0.80, 13, B)), ("extreme", extreme_llrs(n, B, 11))):
        want = _ref(name, llr, 20, 1, 0.75, early_stop, at=(1, 3))
        for iters in (1, 3, 20):
            _assert_bit_exact(_decode(name, llr, iters, "minsum", 0.75, early_stop), want[iters], (name, kind, iters))


def test_no_iteration_and_no_outputs(torch):
    """max_iters = 0 returns the channel values (-0 kept) with its = 0; post / hard may be None."""
    from iib_project_ldpc_codes_amd import decoder
    name = "r36_600"
    llr = extreme_llrs(graph(name).n, B, 11)
    post, hard, its = _decode(name, llr, 0, "minsum", 0.75, True)
    np.testing.assert_array_equal(post.view(np.uint32), llr.view(np.uint32))
    np.testing.assert_array_equal(hard, llr < 0)
    assert np.all(its == 0)
    t = torch.from_numpy(llr).cuda()
    post, hard, its = decoder.bp_decode_dev(graph(name), t, 3, "minsum", 0.75, True, want_post=False, schedule="layered")
    torch.cuda.synchronize()
    want = _ref(name, llr, 3, 1, 0.75, True)
    assert post is None
    np.testing.assert_array_equal(hard.cpu().numpy(), want[1])
    np.testing.assert_array_equal(its.cpu().numpy(), want[2])


# ----------------------------------------- more codewords than workgroups
def test_more_codewords_than_workgroups(torch):
    """B = 264 on a grid capped at 256 workgroups with one slab each: eight workgroups decode a
    second codeword on the slab (and LDS) their first one used."""
    name, frames = "r58_8800", 264
    for p in _routed(name, [(1, 0, 0, 1, 3, frames), (1, 1, 0, 1, 3, frames)], False):
        assert p["grid"] == 256 and p["slab"] > 0, p
    llr = _awgn(graph(name).n, 0.90, 22, frames)
    for early_stop in (False, True):
        want = _ref(name, llr, 3, 1, 0.75, early_stop)
        _assert_bit_exact(_decode(name, llr, 3, "minsum", 0.75, early_stop), want, (name, early_stop))


# ------------------------------------------ a layer larger than the workgroup
@pytest.mark.parametrize("n,threads,lds", [(5060, 256, True), (20270, 1024, False)])
def test_layer_larger_than_the_workgroup(torch, n, threads, lds):
    name = "r36_%d" % n
    calls = [(1, 0, 0, 1, 2, 8), (1, 1, 0, 1, 2, 8)]
    for p in _routed(name, calls, lds):
        assert p["threads"] == threads
    L, layer = layers(name)
    assert np.bincount(layer).max() >= 1.10 * threads
    rc, _, smaller = schedule(graph_csr("r36_%d" % (n - 2)))  # the next smaller (3,6) size falls short
    assert rc == 0 and np.bincount(smaller).max() < 1.10 * threads
    llr = _awgn(n, 0.80, 13, 8)
    for early_stop in (False, True):
        want = _ref(name, llr, 2, 1, 0.75, early_stop)
        _assert_bit_exact(_decode(name, llr, 2, "minsum", 0.75, early_stop), want, (name, early_stop))


# -------------------------------------------------------------- sum-product
@pytest.mark.parametrize("name,sigma", UNSAT)
def test_spa_unsaturated_posterior_tolerance(torch, name, sigma):
    frames = 8
    _routed(name, [(0, 0, 0, 1, it, frames) for it in (1, 3, 5)], True)
    llr = _awgn(graph(name).n, sigma, 21, frames)
    want = _ref(name, llr, 5, 0, at=(1, 3))
    stats = {"graph": name, "kernel": kernel_name(graph_csr(name), True), "sigma": sigma}
    got = {}
    for iters in (1, 3, 5):
        post, hard, its = _decode(name, llr, iters, "spa")
        assert np.abs(want[iters][0]).max() < XMAX  # the case is what it claims: nothing at the clamp
        stats["iters%d" % iters] = _spa_margins(post, want[iters][0])
        got[iters] = (post, its)
    _dump("layered_spa_unsat_" + name, stats)
    for iters, (post, its) in got.items():
        np.testing.assert_allclose(post, want[iters][0], rtol=SPA_RTOL, atol=SPA_ATOL, err_msg=str(stats))
        assert np.all(its == iters)


@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("name,sigma", SATURATED)
def test_spa_saturated(torch, name, sigma, early_stop):
    frames = 32
    lds = name in LDS_GRAPHS
    _routed(name, [(0, int(early_stop), 0, 1, it, frames) for it in (3, 10)], lds)
    llr = _awgn(graph(name).n, sigma, 3, frames)
    want = _ref(name, llr, 10, 0, 1.0, early_stop, at=(3,))
    stats = {"graph": name, "kernel": kernel_name(graph_csr(name), lds), "sigma": sigma, "early_stop": early_stop}
    got = {}
    for iters in (3, 10):
        post, hard, its = _decode(name, llr, iters, "spa", 1.0, early_stop)
        rpost, rhard, rits, _ = want[iters]
        s = _spa_margins(post, rpost)
        s["its_equal_frac"] = float(np.mean(its == rits))
        s["ref_fer"] = float(rhard.any(axis=1).mean())
        stats["iters%d" % iters] = s
        got[iters] = (post, hard, its)
    _dump("layered_spa_sat_%s_sigma%.2f_%s" % (name, sigma, "es" if early_stop else "fixed"), stats)
    assert stats["iters10"]["ref_fer"] == 0.0, stats  # the reference decodes every frame ...
    assert max(stats["iters%d" % it]["ref_post_max_abs"] for it in (3, 10)) > XMAX, stats  # ... saturated
    for iters, (post, hard, its) in got.items():
        rpost, rhard, rits, _ = want[iters]
        assert np.isfinite(post).all(), stats
        d = np.abs(post.astype(np.float64) - rpost)
        assert np.all(d <= SAT_ATOL + SAT_RTOL * np.abs(rpost)), stats
        diff = hard != rhard
        assert np.all(np.abs(rpost[diff]) <= SAT_ATOL), (iters, int(diff.sum()), stats)
        if early_stop:
            assert np.mean(its == rits) >= 0.98, stats
        else:
            assert np.all(its == iters)


# --------------------------------------------------------------- Monte-Carlo
MC_B, MC_ITERS = 128, 20


def _mc_counters(name, channel, p, seed, algo, alpha, early_stop, expurgation=-1, stop=0):
    import torch
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    mc = MonteCarlo(graph(name), channel, p, MC_ITERS, algo=algo, alpha=alpha, early_stop=early_stop, seed=seed,
                    batch=MC_B, expurgation=expurgation, schedule="layered")
    mc.run_batch(0, MC_B, stop)
    torch.cuda.synchronize()
    return mc.counters.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mc_ref_minsum(name, p, early_stop):
    llr = oracle.channel(oracle.CH_BSC, p, 8, 0, graph(name).n, MC_B)
    _, _, its, curve = _ref(name, llr, MC_ITERS, 1, 0.75, early_stop)
    return its, curve


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name,p", [("r36_600", 0.07), ("r58_320", 0.07), ("mixA", 0.12)])
def test_mc_minsum_bsc_exact(torch, name, p, early_stop):
    _routed(name, [(1, int(early_stop), 1, 0, MC_ITERS, MC_B)], True)
    got = _mc_counters(name, "bsc", p, 8, "minsum", 0.75, early_stop)
    want = layered_ref.mc_counters(*_mc_ref_minsum(name, p, early_stop)[::-1])
    assert want[0] == MC_B and 0 < want[1] < MC_B  # both decoded and failed frames
    np.testing.assert_array_equal(got, want)


def test_mc_minsum_expurgation_and_stop_inside_the_batch(torch):
    """X = 3 drops mixA's trial that ends with 3 wrong bits; the tenth frame error ends the batch
    early (the reference alone says so)."""
    name, p, X, stop = "mixA", 0.12, 3, 10
    _routed(name, [(1, 1, 1, 0, MC_ITERS, MC_B)], True)
    its, curve = _mc_ref_minsum(name, p, True)
    want = layered_ref.mc_counters(curve, its, X, stop)
    final = curve[:, -1]
    assert np.any((final > 0) & (final <= X)) and want[1] == stop and want[0] < MC_B
    got = _mc_counters(name, "bsc", p, 8, "minsum", 0.75, True, expurgation=X, stop=stop)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name,sigma", [("r510_640", 0.77), ("mixA", 1.05)])
def test_mc_spa_awgn_vs_reference(torch, name, sigma, early_stop):
    _routed(name, [(0, int(early_stop), 1, 0, MC_ITERS, MC_B)], True)
    got = _mc_counters(name, "awgn", sigma, 31, "spa", 1.0, early_stop)
    llr = oracle.channel(oracle.CH_AWGN, sigma, 31, 0, graph(name).n, MC_B)
    _, h, its, _ = _ref(name, llr, MC_ITERS, 0, 1.0, early_stop)
    fe, be, ti = int(h.any(axis=1).sum()), int(h.sum()), int(its.sum())
    _dump("layered_mc_spa_%s_%s" % (name, "es" if early_stop else "fixed"),
          {"graph": name, "sigma": sigma, "counters_gpu": got[:4].tolist(), "counters_ref": [MC_B, fe, be, ti]})
    assert 0 < fe < MC_B  # both decoded and failed frames at this sigma
    assert got[0] == MC_B
    assert abs(int(got[1]) - fe) <= 2, (got[:4], fe, be, ti)
    assert abs(int(got[2]) - be) <= 0.02 * be + 20, (got[:4], fe, be)
    assert abs(int(got[3]) - ti) <= 0.005 * ti + 2, (got[:4], ti)
    assert got[4] == int((llr < 0).sum())  # channel errors: bit-exact (Philox + fused channel)
    assert got[4 + MC_ITERS] == got[2]  # the last curve point is the final error count


def test_mc_refuses_what_the_schedule_does_not_cover(torch):
    from iib_project_ldpc_codes_amd import _native
    g = graph("r36_600")
    counters = torch.zeros(4 + 6, dtype=torch.int64, device="cuda")
    rc = _native.lib().ldpc_mc_layered_batch_dev(g.handle(), _native.CH_BEC, 0.4, 1, 0, 8, 5, 1, 0.75, 1, -1, 0,
                                                 counters.data_ptr(), None)
    assert rc == _native.LDPC_EINVAL


# ------------------------------------------------------ flooding is untouched
@pytest.mark.parametrize("name", ["r36_600", "r58_8800"])
def test_flooding_argument_is_the_default(torch, name):
    from iib_project_ldpc_codes_amd import decoder
    g = graph(name)
    llr = _awgn(g.n, 0.80, 13, B)
    for algo, alpha in (("minsum", 0.75), ("spa", 1.0)):
        for early_stop in (False, True):
            a = decoder.bp_decode(g, llr, 5, algo, alpha, early_stop)
            b = decoder.bp_decode(g, llr, 5, algo, alpha, early_stop, schedule="flooding")
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
    with pytest.raises(ValueError):
        decoder.bp_decode(g, llr, 5, "spa", schedule="serial")


# ------------------------------------------------------------------- snapshot
def test_snapshot_joins_two_layered_runs(torch, tmp_path):
    from iib_project_ldpc_codes_amd import snapshot
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo

    def mc(schedule="layered"):
        return MonteCarlo(graph("r36_600"), "bsc", 0.07, MC_ITERS, algo="minsum", alpha=0.75, seed=8, batch=64,
                          schedule=schedule)
    whole = mc().run(128, stop_frame_errors=0)
    first = mc()
    path = str(tmp_path / "layered.json")
    first.run(64, stop_frame_errors=0, checkpoint=path)
    snap = snapshot.load(path)
    assert snap["config"]["schedule"] == "layered" and snap["config"]["layer_rule"] == snapshot.LAYER_RULE
    second = mc()
    second.restore(snap)
    joined = second.run(128, stop_frame_errors=0)
    np.testing.assert_array_equal(joined["raw_counters"], whole["raw_counters"])
    its, curve = _mc_ref_minsum("r36_600", 0.07, True)
    np.testing.assert_array_equal(whole["raw_counters"], layered_ref.mc_counters(curve, its))
    with pytest.raises(ValueError):
        mc("flooding").restore(snap)
    flood = mc("flooding")
    assert "schedule" not in snapshot.config(flood)
    with pytest.raises(ValueError):
        mc().restore(flood.snapshot())
