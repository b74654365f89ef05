"""Every fused channel and sampler at 64-bit trial indices, graph indices and seeds: each kernel that
splits seed / first_cw / first_graph into Philox words runs a small batch that straddles 2^32 under
SEED = 0x9E3779B97F4A7C15 (both halves non-zero, bit 63 set) and is compared bit for bit with the
oracle run at the same 64-bit indices.  Everything compared is integer-exact (BEC, BSC, min-sum,
graphs); the stand-alone BI-AWGN channel keeps tests/test_gpu_parity.py::test_channels_vs_oracle's
1e-5 (1 + |x|).

The cases and their oracle side are tests/index64_util.py's; tests/test_index64_ref.py holds every
one of them, on the CPU, to telling a dropped high index word, a high word taken from the first
index without the carry, and a dropped high seed word from the truth.  Each case first holds the
launch plan of its own call to the kernel name it claims, then goes through the public Python API.
Soft decoders: BSC, normalised min-sum alpha = 0.75, 5 iterations, fixed count and early stop.
"""
import numpy as np
import pytest

from tests import index64_util as u
from tests.graph_util import BEC_ENS_MC, BEC_MC, bec_plans, bp_plans
from tests.index64_util import ALPHA, ITERS, SEED, T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


def _ids(cases):
    return [c["name"] for c in cases]


def _counters(torch, mc, first, B, stop=0):
    mc.run_batch(first, B, stop)
    torch.cuda.synchronize()
    return mc.counters.cpu().numpy()


# ---------------------------------------------------------------- stand-alone channel
@pytest.mark.parametrize("c", u.CHANNEL_CASES, ids=_ids(u.CHANNEL_CASES))
def test_channel(torch, c):
    from iib_project_ldpc_codes_amd import decoder
    want = u.want(c)[0]
    got = decoder.channel_dev(c["kind"], c["p"], SEED, c["first"], c["n"], c["B"]).cpu().numpy()
    if c["kind"] == "awgn":
        assert np.all(np.abs(got - want) <= 1e-5 * (1 + np.abs(want)))
    else:
        np.testing.assert_array_equal(got.astype(want.dtype), want)


# ------------------------------------------------------------------- BEC Monte-Carlo
@pytest.mark.parametrize("c", u.BEC_CASES, ids=_ids(u.BEC_CASES))
def test_bec_mc(torch, c):
    """bec_mc_bits_kernel: one codeword per ballot lane, so trials on both sides of 2^32 share a
    plane word; bec_kernel<1024> with the fused channel at n = 107,000."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    n, B, first = c["n"], c["B"], c["first"]
    plan = bec_plans(n, n // 2, [(BEC_MC, B, u.BEC_ITERS)])[0]
    assert plan["name"] == c["kernel"]
    off = T - first
    assert 0 < off < B
    if "bits" in c["kernel"]:
        cw, bits = plan["cw_per_wg"], plan["cw_per_wg"] // plan["W"]
        assert off // cw >= 1 and (off % cw) % bits != 0, (off, plan)  # inside a plane word of a later workgroup
    want, stop = u.want(c)
    stop = int(stop[0])
    if c["stop_after"] is not None:
        assert want[1] == stop > 0 and want[0] < B and first + int(want[0]) - 1 >= T
    g = u.new_graph(("reg", n, 11))
    mc = MonteCarlo(g, "bec", u.EPS, u.BEC_ITERS, expurgation=c["X"], seed=SEED, batch=B)
    np.testing.assert_array_equal(_counters(torch, mc, first, B, stop), want)


@pytest.mark.parametrize("c", u.BEC_ENS_CASES, ids=_ids(u.BEC_ENS_CASES))
def test_bec_ensemble_mc(torch, c):
    """Trial t decodes on graph t with channel word t: trial by trial (curves and iteration counts),
    then the B trials as one batch (tests/test_gpu_bec_plan.py::test_ensemble_mc)."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    n, B, first = c["n"], c["B"], c["first"]
    assert {p["name"] for p in bec_plans(n, n // 2, [(BEC_ENS_MC, b, u.BEC_ITERS) for b in (1, B)])} == {c["kernel"]}
    want_c, want_i = u.want(c)
    mc = MonteCarlo.ensemble(n, 3, 6, "bec", u.EPS, u.BEC_ITERS, seed=SEED, batch=1, expurgation=-1)
    prev = mc.counters.cpu().numpy().copy()
    for t in range(B):
        cur = _counters(torch, mc, first + t, 1).copy()
        d = cur - prev
        prev = cur
        assert d[0] == 1 and d[3] == want_i[t], (t, d[:4])
        np.testing.assert_array_equal(d[4:], want_c[t], err_msg="trial %d" % (first + t))
    mc = MonteCarlo.ensemble(n, 3, 6, "bec", u.EPS, u.BEC_ITERS, seed=SEED, batch=B, expurgation=-1)
    got = _counters(torch, mc, first, B)
    np.testing.assert_array_equal(got, u.counters(want_c, want_i))


# ------------------------------------------------------------------- soft Monte-Carlo
def _fixed_graph(c, monkeypatch):
    """The case's graph with its device layout built under the case's environment, and the plan's
    environment to match."""
    if c["noloc"]:
        monkeypatch.setenv("LDPC_NO_LOC_LAYOUT", "1")
    else:
        monkeypatch.delenv("LDPC_NO_LOC_LAYOUT", raising=False)
    g = u.new_graph(c["graph"])
    g.handle()
    return g, {"LDPC_NO_LOC_LAYOUT": "1"} if c["noloc"] else None


@pytest.mark.parametrize("c", u.SOFT_CASES, ids=_ids(u.SOFT_CASES))
def test_flooding_minsum_mc(torch, monkeypatch, c):
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    g, env = _fixed_graph(c, monkeypatch)
    csr = u.fixed_graph(c["graph"])[1]
    for es, want in zip(u.MODES, u.want(c)):
        assert bp_plans(csr, [(1, int(es), 1, 0, ITERS, c["B"])], env=env)[0]["name"] == c["kernel"]
        mc = MonteCarlo(g, "bsc", c["p"], ITERS, algo="minsum", alpha=ALPHA, early_stop=es, seed=SEED, batch=c["B"])
        np.testing.assert_array_equal(_counters(torch, mc, c["first"], c["B"]), want, err_msg=str(es))


@pytest.mark.parametrize("c", u.SPA_CASES, ids=_ids(u.SPA_CASES))
def test_flooding_spa_mc_channel_stream(torch, monkeypatch, c):
    """The sum-product instantiations (another translation unit, the same staging source), and the
    only Monte-Carlo calls the plan gives to bp_loc_kernel's 256-thread (3,6) and RSU shapes: the
    number of trials and the channel errors, which are the channel stream and need no tolerance."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    g, env = _fixed_graph(c, monkeypatch)
    csr = u.fixed_graph(c["graph"])[1]
    want = u.want(c)[0]
    for es in u.MODES:
        plan = bp_plans(csr, [(0, int(es), 1, 0, ITERS, c["B"])], env=env)[0]
        assert plan["name"] == c["kernel"] and plan["threads"] == c["threads"], plan
        mc = MonteCarlo(g, "bsc", c["p"], ITERS, algo="spa", early_stop=es, seed=SEED, batch=c["B"])
        got = _counters(torch, mc, c["first"], c["B"])
        assert got[0] == want[0] == c["B"]
        assert got[4] == want[1], (es, got[:5])


@pytest.mark.parametrize("c", u.SOFT_ENS_CASES, ids=_ids(u.SOFT_ENS_CASES))
def test_ensemble_minsum_mc(torch, c):
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    from tests.test_ens_plan import ens_plans
    for es, want in zip(u.MODES, u.want(c)):
        rc, plans = ens_plans(*c["shape"], [(1, int(es), 1, 0, ITERS, c["B"])])
        assert rc == 0 and plans[0]["name"] == c["kernel"]
        mc = MonteCarlo.ensemble(*c["shape"], "bsc", c["p"], ITERS, algo="minsum", alpha=ALPHA, early_stop=es,
                                 seed=SEED, batch=c["B"])
        np.testing.assert_array_equal(_counters(torch, mc, c["first"], c["B"]), want, err_msg=str(es))


@pytest.mark.parametrize("c", u.LAYER_CASES, ids=_ids(u.LAYER_CASES))
def test_layered_minsum_mc(torch, c):
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    from tests import layered_util
    csr = layered_util.graph_csr(c["graph"])
    for es, want in zip(u.MODES, u.want(c)):
        p = layered_util.layer_plans(csr, [(1, int(es), 1, 0, ITERS, c["B"])])[0]
        assert p["name"] == layered_util.kernel_name(csr, c["lds"]) == c["kernel"]
        if not c["lds"]:
            assert 0 < p["lds_slots"] < csr[2].size - 1 + csr[1].size, p  # words really stored in the slab
        mc = MonteCarlo(layered_util.graph(c["graph"]), "bsc", c["p"], ITERS, algo="minsum", alpha=ALPHA,
                        early_stop=es, seed=SEED, batch=c["B"], schedule="layered")
        np.testing.assert_array_equal(_counters(torch, mc, c["first"], c["B"]), want, err_msg=str(es))


def _layer_q_mc(c, es, batch):
    from iib_project_ldpc_codes_amd.decoder import Quant
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    from tests import layered_util
    return MonteCarlo(layered_util.graph(c["graph"]), "bsc", c["p"], ITERS, algo="minsum", early_stop=es, seed=SEED,
                      batch=batch, schedule="layered", quant=Quant(*u.QUANT))


def _layer_q_routed(c, es, B):
    from tests import layered_q_util, layered_util
    csr = layered_util.graph_csr(c["graph"])
    p = layered_q_util.layer_q_plans(csr, [(1, int(es), 1, 0, ITERS, B)])[0]
    assert p["name"] == layered_q_util.kernel_name(csr), p
    return p["name"]


@pytest.mark.parametrize("c", u.LAYER_Q_CASES, ids=_ids(u.LAYER_Q_CASES))
def test_layered_q_mc(torch, c):
    for es, want in zip(u.MODES, u.want(c)):
        assert _layer_q_routed(c, es, c["B"]) == c["kernel"]
        got = _counters(torch, _layer_q_mc(c, es, c["B"]), c["first"], c["B"])
        np.testing.assert_array_equal(got, want, err_msg=str(es))


# ---------------------------------------------------------------------- ML Monte-Carlo
@pytest.mark.parametrize("c", u.ML_CASES, ids=_ids(u.ML_CASES))
def test_ml_mc(torch, c):
    """ldpc_mc_ml_batch_dev: message passing and ML decoding of the same channel word (and, in
    ensemble mode, on the same graph t)."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    want = u.want(c)[0]
    kw = dict(seed=SEED, batch=c["B"], optimal=True, message_passing=True)
    if c["ens"]:
        mc = MonteCarlo.ensemble(c["n"], 3, 6, "bec", u.ML_EPS, u.ML_ITERS, **kw)
    else:
        mc = MonteCarlo(u.new_graph(("reg", c["n"], 9)), "bec", u.ML_EPS, u.ML_ITERS, **kw)
    mc.run_batch(c["first"], c["B"], 0)
    torch.cuda.synchronize()
    res = mc.results()
    got = [res["num_tests"], res["frame_errors"], res["bit_errors"], res["ml_frame_errors"], res["ml_bit_errors"]]
    assert res["ml_num_tests"] == c["B"]
    np.testing.assert_array_equal(np.concatenate([got, res["raw_counters"][4:]]), want)


# ---------------------------------------------------------------------------- samplers
@pytest.mark.parametrize("c", u.SAMPLER_CASES, ids=_ids(u.SAMPLER_CASES))
def test_samplers(torch, c):
    """Graphs first_graph .. straddling 2^32 (G = 300: the sequential sampler's search pass scans its
    per-graph state 256 graphs at a time, with g on both sides) through the host-array and the
    device-pointer entries; graphs and attempt counts against the oracle."""
    from iib_project_ldpc_codes_amd import _native
    L = _native.lib()
    G, first = c["B"], c["first"]
    want = u.want(c)
    assert np.all(want[2] > 0)
    if c["kind"] == "csr":
        vptr, cptr = u.csr_ptrs(c["n"])
        E = int(vptr[-1])
        a, b, att = np.zeros((G, E), np.int32), np.zeros((G, E), np.int32), np.zeros(G, np.int32)
        rc = L.ldpc_sample_csr(c["n"], len(cptr) - 1, vptr.ctypes.data, cptr.ctypes.data, SEED, first, G, a.ctypes.data,
                               b.ctypes.data, att.ctypes.data)
        _native.check(rc, "ldpc_sample_csr")
        for got, w in zip((a, b, att), want):
            np.testing.assert_array_equal(got, w)
        return
    n, dv, dc = c["n"], c["dv"], c["dc"]
    E = n * dv
    if "seq" in c["name"]:
        assert E >= u.SEQ_E and (n != 2732 or E == 8196)
    else:
        assert E < u.SEQ_E
    a, b, att = np.zeros((G, E), np.int32), np.zeros((G, E), np.int32), np.zeros(G, np.int32)
    _native.check(L.ldpc_sample_regular(n, dv, dc, SEED, first, G, a.ctypes.data, b.ctypes.data, att.ctypes.data),
                  "ldpc_sample_regular")
    for got, w in zip((a, b, att), want):
        np.testing.assert_array_equal(got, w)
    da = torch.zeros((G, E), dtype=torch.int32, device="cuda")
    db, datt = torch.zeros_like(da), torch.zeros(G, dtype=torch.int32, device="cuda")
    rc = L.ldpc_sample_regular_dev(n, dv, dc, SEED, first, G, da.data_ptr(), db.data_ptr(), datt.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "ldpc_sample_regular_dev")
    torch.cuda.synchronize()
    for got, w in zip((da, db, datt), want):
        np.testing.assert_array_equal(got.cpu().numpy(), w)


# ------------------------------------------------------------------------ driver level
def test_restored_run_crosses_2_32(torch):
    """MonteCarlo.run restored to trial_base = 2^32 - 96, three rounds of 64: the oracle's counters
    over [2^32 - 96, 2^32 + 96), and the same trials as one batch."""
    c = u.DRIVER_CASE
    first, want = c["first"], u.want(c)[1]
    assert _layer_q_routed(c, True, 64) == _layer_q_routed(c, True, 192) == "bp_layer_q_kernel<8>"
    mc = _layer_q_mc(c, True, 64)
    snap = mc.snapshot()
    snap["trial_ranges"] = [[first, first]]
    mc.restore(snap)
    res = mc.run(192, stop_frame_errors=0)
    assert mc.rounds == 3 and mc.next_trial() == T + 96
    assert mc.snapshot()["trial_ranges"] == [[T - 96, T + 96]]
    np.testing.assert_array_equal(res["raw_counters"], want)
    np.testing.assert_array_equal(_counters(torch, _layer_q_mc(c, True, 192), first, 192), want)
