"""bp_layer_q_kernel (csrc/bp_layer_q.hip), the fixed-point layered min-sum with compressed check
records, against the numpy reference of its contract (tests/layered_q_ref.py, the per-edge form;
the layers from ldpc_debug_layer_schedule).  Every value is an integer: post, hard and its are
bit-exact or wrong.

Every case first holds the launch plan of its own calls (layer_q_plans) to the kernel name it
claims, bp_layer_q_kernel<8|16|32>.

* Decodes: 1 / 3 / 20 iterations, fixed count and early stop, on 24 BI-AWGN frames (sigma 0.80,
  seed 13) and graph_util.extreme_llrs (NaN added: NaN, +-inf, -0 and denormals through the
  quantiser), for five parameter sets on (3,6) n = 600, n = 602 (P padded), r58_320 (variable
  degree 5), r510_640 (16 wide), r324_1024 (32 wide, 8-byte records), mixA / mixB (mixed degrees)
  and (3,6) n = 5,060 (a layer of 282 checks on 256 threads).  One reference run per graph, set,
  frame set and mode: a decode of t iterations is a prefix of the 20-iteration one.  The sets that
  claim clamping posteriors are held to it from the reference (saturation events > 0 and
  max |P| = Pmax on the graphs named in CLAMPS).
* Boundary calls: max_iters = 0, want_post=False, B = 0, B = 1 (the plan's grid is always B).
* Fused Monte-Carlo on the BSC: every counter and the whole curve bit-exact, one case with
  expurgation and a stop_frame_errors cut inside the batch.
* Fused Monte-Carlo on BI-AWGN: the device channel is within 1e-5 relative of the oracle's, not
  bit-equal, so a quantiser boundary can move: tests/test_gpu_layered.py::
  test_mc_spa_awgn_vs_reference's tolerances, margins dumped.
* Refusals, and calls without quant are what they were.
"""
import ctypes as ct
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import layered_q_ref
from tests.graph_util import extreme_llrs
from tests.layered_util import graph, graph_csr, layers, schedule
from tests.layered_q_util import kernel_name, layer_q_plans
from tests.test_gpu_fullsize import _dump

pytestmark = pytest.mark.gpu

B = 24
GRAPHS = ["r36_600", "r36_602", "r58_320", "r510_640", "r324_1024", "mixA", "mixB", "r36_5060"]
WIDTH = {"r36_600": 8, "r36_602": 8, "r58_320": 8, "r510_640": 16, "r324_1024": 32, "mixA": 8, "mixB": 32,
         "r36_5060": 8}
# bits, post_bits, scale, norm8, offset
SETS = [(6, 8, 2.0, 6, 0), (7, 8, 4.0, 6, 0), (6, 6, 2.0, 6, 0), (4, 6, 0.5, 8, 1), (2, 2, 0.25, 8, 0)]
# the sets whose posteriors clamp, and the graphs on which the AWGN frames make them (the check
# degree 24 and 32 graphs' messages stay small)
CLAMPS = {(7, 8, 4.0, 6, 0): ("r36_600", "r36_602", "r58_320", "r510_640", "mixA", "r36_5060"),
          (6, 6, 2.0, 6, 0): ("r36_600", "r36_602", "r58_320", "r510_640", "mixA", "mixB", "r36_5060")}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


def _quant(params):
    from iib_project_ldpc_codes_amd.decoder import Quant
    return Quant(*params)


def _routed(name, calls):
    """The plans of `calls` (algo, early_stop, mc, want_post, iters, B) on graph `name`, each
    held to the width the case claims."""
    csr = graph_csr(name)
    plans = layer_q_plans(csr, calls)
    for call, p in zip(calls, plans):
        assert p["name"] == kernel_name(csr) == "bp_layer_q_kernel<%d>" % WIDTH[name], (name, call, p)
        assert p["grid"] == call[5] and p["threads"] == 256, (name, call, p)
    return plans


def _decode(name, llr, iters, params, early_stop=False):
    from iib_project_ldpc_codes_amd import decoder
    return decoder.bp_decode(graph(name), llr, iters, "minsum", 1.0, early_stop, schedule="layered",
                             quant=_quant(params))


def _ref(name, llr, iters, params, early_stop=False, at=()):
    return layered_q_ref.decode(graph_csr(name), layers(name)[1], llr, iters, *params, early_stop=early_stop, at=at)


def _assert_bit_exact(got, want, what):
    post, hard, its = got
    assert post.dtype == np.int8 and hard.dtype == np.uint8 and its.dtype == np.int32
    np.testing.assert_array_equal(hard, want[1], err_msg=str(what))
    np.testing.assert_array_equal(its, want[2], err_msg=str(what))
    np.testing.assert_array_equal(post, want[0], err_msg=str(what))


@functools.lru_cache(maxsize=None)
def _frames(n, kind):
    if kind == "awgn":
        return oracle.channel(oracle.CH_AWGN, 0.80, 13, 0, n, B)
    llr = extreme_llrs(n, B, 11)
    llr[:, 1::97] = np.nan
    llr[:, 2::89] = np.float32(1e-40)  # a denormal
    llr[:, 3::83] = np.float32(-1e-40)
    llr[:, 4::79] = np.inf
    llr[:, 5::73] = -np.inf
    return llr


# ------------------------------------------------------------------- decodes
@pytest.mark.parametrize("params", SETS)
@pytest.mark.parametrize("name", GRAPHS)
def test_bit_exact(torch, name, params):
    n = graph(name).n
    _routed(name, [(1, es, 0, 1, it, B) for es in (0, 1) for it in (1, 3, 20)])
    if name == "r36_5060":  # a layer larger than the workgroup; the next smaller (3,6) size falls short
        assert np.bincount(layers(name)[1]).max() >= 1.10 * 256
        rc, _, smaller = schedule(graph_csr("r36_5058"))
        assert rc == 0 and np.bincount(smaller).max() < 1.10 * 256
    for kind in ("awgn", "extreme"):
        llr = _frames(n, kind)
        for early_stop in (False, True):
            want = _ref(name, llr, 20, params, early_stop, at=(1, 3))
            if kind == "awgn" and not early_stop and name in CLAMPS.get(params, ()):
                Pmax = (1 << (params[1] - 1)) - 1  # the case is what it claims
                assert want[20][4] > 0 and np.abs(want[20][0].astype(np.int32)).max() == Pmax
            for iters in (1, 3, 20):
                _assert_bit_exact(_decode(name, llr, iters, params, early_stop), want[iters],
                                  (name, params, kind, early_stop, iters))


def test_boundary_calls(torch):
    """max_iters = 0 returns the quantised channel values with its = 0; post may be None; B = 0
    does nothing; B = 1."""
    from iib_project_ldpc_codes_amd import decoder
    name, params = "r36_602", (6, 8, 2.0, 6, 0)
    g, q = graph(name), _quant(params)
    llr = _frames(g.n, "extreme")
    _routed(name, [(1, 1, 0, 1, 0, B), (1, 1, 0, 0, 3, B), (1, 0, 0, 1, 3, 1)])
    post, hard, its = _decode(name, llr, 0, params, True)
    c = layered_q_ref.quantise(llr, params[2], q.Q)
    np.testing.assert_array_equal(post, c)
    np.testing.assert_array_equal(hard, c < 0)
    assert np.all(its == 0) and post.dtype == np.int8
    t = torch.from_numpy(llr).cuda()
    post, hard, its = decoder.bp_decode_dev(g, t, 3, "minsum", 1.0, True, want_post=False, schedule="layered", quant=q)
    torch.cuda.synchronize()
    want = _ref(name, llr, 3, params, True)
    assert post is None
    np.testing.assert_array_equal(hard.cpu().numpy(), want[1])
    np.testing.assert_array_equal(its.cpu().numpy(), want[2])
    post, hard, its = decoder.bp_decode_dev(g, t, 3, "minsum", 1.0, False, want_hard=False, schedule="layered", quant=q)
    torch.cuda.synchronize()
    assert hard is None
    np.testing.assert_array_equal(post.cpu().numpy(), _ref(name, llr, 3, params)[0])
    post, hard, its = decoder.bp_decode_dev(g, t[:0], 3, "minsum", schedule="layered", quant=q)
    torch.cuda.synchronize()
    assert post.shape == (0, g.n) and its.shape == (0,)
    _assert_bit_exact(_decode(name, llr[:1], 3, params), _ref(name, llr[:1], 3, params), "B = 1")


# --------------------------------------------------------------- Monte-Carlo
MC_B, MC_ITERS = 128, 20


def _mc(name, channel, p, seed, params, early_stop, expurgation=-1, batch=MC_B, schedule="layered"):
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    return MonteCarlo(graph(name), channel, p, MC_ITERS, algo="minsum", early_stop=early_stop, seed=seed, batch=batch,
                      expurgation=expurgation, schedule=schedule, quant=None if params is None else _quant(params))


def _mc_counters(name, channel, p, seed, params, early_stop, expurgation=-1, stop=0):
    import torch
    mc = _mc(name, channel, p, seed, params, early_stop, expurgation)
    mc.run_batch(0, MC_B, stop)
    torch.cuda.synchronize()
    return mc.counters.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mc_ref_bsc(name, p, params, early_stop):
    llr = oracle.channel(oracle.CH_BSC, p, 8, 0, graph(name).n, MC_B)
    _, _, its, curve, _ = _ref(name, llr, MC_ITERS, params, early_stop)
    return its, curve


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name,p,params", [("r36_600", 0.07, (6, 8, 2.0, 6, 0)), ("r36_600", 0.07, (4, 6, 1.0, 8, 1)),
                                           ("mixA", 0.12, (6, 8, 2.0, 6, 0))])
def test_mc_bsc_exact(torch, name, p, params, early_stop):
    _routed(name, [(1, int(early_stop), 1, 0, MC_ITERS, MC_B)])
    got = _mc_counters(name, "bsc", p, 8, params, early_stop)
    want = layered_q_ref.mc_counters(*_mc_ref_bsc(name, p, params, early_stop)[::-1])
    assert want[0] == MC_B and 0 < want[1] < MC_B  # both decoded and failed frames
    np.testing.assert_array_equal(got, want)


def test_mc_expurgation_and_stop_inside_the_batch(torch):
    """X = 3 drops mixA's trial that ends with 1 wrong bit; the tenth frame error ends the batch
    early (the reference alone says so)."""
    name, p, params, X, stop = "mixA", 0.12, (6, 8, 2.0, 6, 0), 3, 10
    _routed(name, [(1, 1, 1, 0, MC_ITERS, MC_B)])
    its, curve = _mc_ref_bsc(name, p, params, True)
    want = layered_q_ref.mc_counters(curve, its, X, stop)
    final = curve[:, -1]
    assert np.any((final > 0) & (final <= X)) and want[1] == stop and want[0] < MC_B
    got = _mc_counters(name, "bsc", p, 8, params, True, expurgation=X, stop=stop)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name,sigma", [("r510_640", 0.77), ("mixA", 1.05)])
def test_mc_awgn_vs_reference(torch, name, sigma, early_stop):
    params = (6, 8, 2.0, 6, 0)
    _routed(name, [(1, int(early_stop), 1, 0, MC_ITERS, MC_B)])
    got = _mc_counters(name, "awgn", sigma, 31, params, early_stop)
    llr = oracle.channel(oracle.CH_AWGN, sigma, 31, 0, graph(name).n, MC_B)
    _, h, its, curve, _ = _ref(name, llr, MC_ITERS, params, early_stop)
    fe, be, ti = int(h.any(axis=1).sum()), int(h.sum()), int(its.sum())
    # channel errors c < 0: a device LLR within 1e-5 relative of the oracle's crosses the
    # quantiser's -0.5 boundary only from within that distance of it
    t = llr.astype(np.float64) * params[2]
    near = int((np.abs(t + 0.5) <= 2e-5 * np.abs(t)).sum())
    _dump("layered_q_mc_awgn_%s_%s" % (name, "es" if early_stop else "fixed"),
          {"graph": name, "sigma": sigma, "quant": list(params), "counters_gpu": got[:4].tolist(),
           "counters_ref": [MC_B, fe, be, ti], "curve0_gpu": int(got[4]), "curve0_ref": int(curve[:, 0].sum()),
           "llrs_near_the_sign_boundary": near})
    assert 0 < fe < MC_B  # both decoded and failed frames at this sigma
    assert got[0] == MC_B
    assert abs(int(got[1]) - fe) <= 2, (got[:4], fe, be, ti)
    assert abs(int(got[2]) - be) <= 0.02 * be + 20, (got[:4], fe, be)
    assert abs(int(got[3]) - ti) <= 0.005 * ti + 2, (got[:4], ti)
    assert abs(int(got[4]) - int(curve[:, 0].sum())) <= near
    assert got[4 + MC_ITERS] == got[2]  # the last curve point is the final error count


# ------------------------------------------------------------------ refusals
def test_refusals(torch):
    from iib_project_ldpc_codes_amd import _native, decoder
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    from tests.test_layered_q_ref import INVALID
    L = _native.lib()
    g = graph("r36_600")
    llr = torch.zeros((2, g.n), dtype=torch.float32, device="cuda")
    post = torch.zeros((2, g.n), dtype=torch.int8, device="cuda")
    its = torch.zeros(2, dtype=torch.int32, device="cuda")
    counters = torch.zeros(4 + 6, dtype=torch.int64, device="cuda")

    def decode(graph_, q):
        return L.ldpc_bp_layered_q_decode_batch_dev(graph_.handle(), llr.data_ptr(), 2, 3, q, 0, post.data_ptr(), None,
                                                    its.data_ptr(), None)

    def mc(graph_, channel, param, q):
        return L.ldpc_mc_layered_q_batch_dev(graph_.handle(), channel, param, 1, 0, 8, 5, q, 1, -1, 0,
                                             counters.data_ptr(), None)

    good = _native.Quant(2.0, 6, 8, 6, 0)
    assert decode(g, ct.addressof(good)) == 0 and mc(g, _native.CH_BSC, 0.07, ct.addressof(good)) == 0
    for p in INVALID:
        q = _native.Quant(p[2], p[0], p[1], p[3], p[4])
        assert decode(g, ct.addressof(q)) == _native.LDPC_EINVAL, p
        assert mc(g, _native.CH_BSC, 0.07, ct.addressof(q)) == _native.LDPC_EINVAL, p
    assert decode(g, None) == _native.LDPC_EINVAL
    assert mc(g, _native.CH_BEC, 0.4, ct.addressof(good)) == _native.LDPC_EINVAL
    # a block beyond LDS: (3,6) n = 53,250 (tests/test_layer_q_plan.py: 53,248 is the last that fits)
    big = graph("r36_53250")
    bllr = torch.zeros((1, big.n), dtype=torch.float32, device="cuda")
    rc = L.ldpc_bp_layered_q_decode_batch_dev(big.handle(), bllr.data_ptr(), 1, 3, ct.addressof(good), 0, None, None,
                                              its.data_ptr(), None)
    assert rc == _native.LDPC_EUNSUP
    assert mc(big, _native.CH_BSC, 0.07, ct.addressof(good)) == _native.LDPC_EUNSUP
    torch.cuda.synchronize()
    q = decoder.Quant(6, 8, 2.0)
    for kw in ({"schedule": "flooding", "algo": "minsum"}, {"schedule": "layered", "algo": "spa"}):
        with pytest.raises(ValueError):
            decoder.bp_decode(g, np.zeros((2, g.n), np.float32), 3, quant=q, **kw)
        with pytest.raises(ValueError):
            MonteCarlo(g, "bsc", 0.07, 5, quant=q, **kw)


# ------------------------------------------------- the other paths are untouched
def test_quant_none_is_the_default(torch):
    from iib_project_ldpc_codes_amd import decoder
    g = graph("r36_600")
    llr = _frames(g.n, "awgn")
    for sched in ("flooding", "layered"):
        for algo, alpha in (("minsum", 0.75), ("spa", 1.0)):
            for early_stop in (False, True):
                a = decoder.bp_decode(g, llr, 5, algo, alpha, early_stop, schedule=sched)
                b = decoder.bp_decode(g, llr, 5, algo, alpha, early_stop, schedule=sched, quant=None)
                assert a[0].dtype == np.float32
                for x, y in zip(a, b):
                    np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
    for sched in ("flooding", "layered"):
        from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
        a = MonteCarlo(g, "bsc", 0.07, MC_ITERS, algo="minsum", alpha=0.75, seed=8, batch=MC_B, schedule=sched)
        b = MonteCarlo(g, "bsc", 0.07, MC_ITERS, algo="minsum", alpha=0.75, seed=8, batch=MC_B, schedule=sched,
                       quant=None)
        for m in (a, b):
            m.run_batch(0, MC_B)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(a.counters.cpu().numpy(), b.counters.cpu().numpy())


# ------------------------------------------------------------------- snapshot
def test_snapshot_joins_two_quantised_runs(torch, tmp_path):
    from iib_project_ldpc_codes_amd import snapshot
    params = (6, 8, 2.0, 6, 0)

    def mc(p=params):
        return _mc("r36_600", "bsc", 0.07, 8, p, True, batch=64)
    whole = mc().run(128, stop_frame_errors=0)
    first = mc()
    path = str(tmp_path / "layered_q.json")
    first.run(64, stop_frame_errors=0, checkpoint=path)
    snap = snapshot.load(path)
    assert snap["config"]["quant"] == {"bits": 6, "post_bits": 8, "scale": 2.0, "norm8": 6, "offset": 0}
    assert snap["config"]["schedule"] == "layered"
    second = mc()
    second.restore(snap)
    joined = second.run(128, stop_frame_errors=0)
    np.testing.assert_array_equal(joined["raw_counters"], whole["raw_counters"])
    its, curve = _mc_ref_bsc("r36_600", 0.07, params, True)
    np.testing.assert_array_equal(whole["raw_counters"], layered_q_ref.mc_counters(curve, its))
    with pytest.raises(ValueError):
        mc((6, 8, 2.0, 6, 1)).restore(snap)  # another Quant
    with pytest.raises(ValueError):
        mc(None).restore(snap)               # the fp32 layered decoder
    plain = mc(None)
    assert "quant" not in snapshot.config(plain)
    with pytest.raises(ValueError):
        mc().restore(plain.snapshot())
