"""The device entry points held to what include/ldpc_mi355x.h promises around the kernels: every
`_dev` entry is asynchronous on its `stream` and ordered on it, calls queued on one stream without a
host synchronisation in between see each other's results (the persistent grid's codeword counter,
the sampler's search control, the Monte-Carlo counters with their exact stop), the grow-only
workspaces are per (device, stream), and two host threads can drive two streams at once.

The method (tests/stream_util.py): a bounded stall in front of the work on a side stream.  Whatever
the library issues on another stream, or does when the call is enqueued, runs early and meets
zero-filled inputs, garbage counters and sentinel-filled outputs, and the comparison with the oracle
fails.  Every case first runs a warm-up call of the same shape on the same stream (another seed,
other trials and inputs), so the workspaces are grown and hold stale contents of another call; every
comparison is with the oracle, integer-exact (BEC, BSC, normalised min-sum alpha = 0.75, the
fixed-point layered decoder, samplers, ML), at the shapes of tests/index64_util.py with ordinary
seeds and indices.

Min-sum on the (3,6) n = 1,000 code runs on bp_lds_kernel<3,6> (no persistent grid, no slabs); the
local-edge kernel's persistent counter and per-workgroup slabs are reached by min-sum at n = 10,000
with early stop and posteriors, so the bp_loc cases run there, next to the n = 1,000 ones.
"""
import threading

import numpy as np
import pytest

from oracle import oracle
from tests import index64_util as u
from tests import stream_util as su
from tests.graph_util import BEC_DECODE, BEC_ENS_MC, BEC_MC, bec_plans, bp_plans
from tests.index64_util import ALPHA, ITERS

pytestmark = pytest.mark.gpu

SEED, FIRST = 20261020, 1000          # the calls that are compared
WARM_SEED, WARM_FIRST = 977, 50000    # the warm-up calls of the same shapes
REG1K, REG10K = ("reg", 1000, 25), ("reg", 10000, 25)
P1K, P10K = 0.04, 0.03
ML_DECODE_EPS = 0.46  # some of the 16 words solved, some given up, on both ML decode entries (asserted)
# entries that block the host on purpose, and why (include/ldpc_mi355x.h, "Streams")
BLOCKING = {"sample_csr": "csr_shape_upload synchronises the stream before it rewrites the shape buffer"}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    t.cuda.set_device(0)
    su.calibrate(t)
    return t


def _plan_names(csr, calls, env=None):
    return [p["name"] for p in bp_plans(csr, calls, env=env)]


# ----------------------------------------------------------------------------- premise
def test_side_stream_runs_apart_from_the_null_stream(torch):
    """With the stall queued on a side stream, work on the default stream completes while the
    stall still runs: the side streams neither synchronise with the null stream nor share its
    hardware queue.  Without this the file discriminates nothing."""
    S = su.side_streams(torch)[0]
    x = torch.zeros(1 << 16, device="cuda")
    torch.cuda.synchronize()
    done = su.stall(torch, S)
    x.fill_(3.0)
    torch.cuda.default_stream().synchronize()
    early = done.query()
    S.synchronize()
    assert float(x[0]) == 3.0 and float(x[-1]) == 3.0
    assert not early, "the default stream waited for the stall on the side stream"
    assert done.query()


# ------------------------------------------------------------- 1. late inputs, entry by entry
def _job_channel(torch, seed, first, want):
    from iib_project_ldpc_codes_amd import decoder
    c = u.BY_NAME["channel-bsc"]
    j = su.Job(torch, "channel")
    w = u.expected(c, u.true_indices(first, c["B"]), seed)[0] if want else None
    out = j.output((c["B"], c["n"]), torch.float32, w)
    j.call(lambda s: decoder.channel_dev("bsc", c["p"], seed, first, c["n"], c["B"], out=out, stream=s))
    return [j]


def _job_bec_decode(B, kernel):
    def make(torch, seed, first, want):
        from iib_project_ldpc_codes_amd import decoder
        n, iters = 96, u.BEC_ITERS
        assert bec_plans(n, n // 2, [(BEC_DECODE, B, iters)])[0]["name"] == kernel
        g, _, _ = su.graph(("reg", n, 11))
        words = u.channel_rows(oracle.CH_BEC, u.EPS, seed, u.true_indices(first, B), n)
        j = su.Job(torch, "bec decode B=%d" % B)
        dw = j.late_input(words.astype(np.uint8))
        w = oracle.bec_decode_batch(words, iters, g.variable_lookup, g.check_lookup, n, g.k, 3, 6) if want else (None,) * 3
        j.expect(dw, None if w[0] is None else w[0].astype(np.uint8), "words")
        err = j.accumulator((B, iters), torch.int32, w[1], "errors")
        its = j.output((B,), torch.int32, w[2], "its")
        j.call(lambda s: decoder.bec_decode_dev(g, dw, iters, errors=err, its=its, stream=s))
        return [j]
    return make


def _job_flood(spec, noloc, kernel, p, persistent=False):
    """ldpc_bp_decode_batch_dev, fixed count and early stop with posteriors, behind one stall"""
    def make(torch, seed, first, want):
        g, csr, env = su.graph(spec, noloc)
        plans = bp_plans(csr, [(1, es, 0, 1, ITERS, 8) for es in (0, 1)], env=env)
        assert [q["name"] for q in plans] == [kernel, kernel], plans
        if persistent:  # early stop with posteriors: the grid pulls codewords from a counter behind the slabs
            assert plans[1]["persistent"] == 1 and 0 < plans[1]["slab"] == plans[1]["counter"], plans[1]
        if "slab" in kernel or "gmem" in kernel:
            assert min(q["slab"] for q in plans) > 0, plans
        return [su.decode_job(torch, spec, p, seed, first, 8, ITERS, es, noloc, want) for es in (False, True)]
    return make


def _layered_jobs(torch, name, quant, seed, first, want):
    from iib_project_ldpc_codes_amd import decoder
    from tests import layered_q_ref, layered_ref, layered_util
    csr, layer = layered_util.graph_csr(name), layered_util.layers(name)[1]
    g = layered_util.graph(name)
    g.handle()
    n, B = g.n, 8
    llr_h = u.channel_rows(oracle.CH_BSC, 0.06, seed, u.true_indices(first, B), n)
    jobs = []
    for es in (False, True):
        j = su.Job(torch, "layered%s %s es=%d" % ("_q" if quant else "", name, es))
        llr = j.late_input(llr_h)
        w = (None,) * 3
        if want and quant:
            w = layered_q_ref.decode(csr, layer, llr_h, ITERS, *u.QUANT, early_stop=es)[:3]
        elif want:
            w = layered_ref.decode(csr, layer, llr_h, ITERS, 1, ALPHA, es)[:3]
        post = j.output((B, n), torch.int8 if quant else torch.float32, w[0], "post")
        hard = j.output((B, n), torch.uint8, w[1], "hard")
        its = j.output((B,), torch.int32, w[2], "its")
        q = decoder.Quant(*u.QUANT) if quant else None
        j.call(lambda s, es=es, llr=llr, post=post, hard=hard, its=its: decoder.bp_decode_dev(
            g, llr, ITERS, "minsum", ALPHA, es, post=post, hard=hard, its=its, stream=s, schedule="layered", quant=q))
        jobs.append(j)
    return jobs


def _job_layered(torch, seed, first, want):
    from tests import layered_util
    csr = layered_util.graph_csr("r36_600")
    assert [q["name"] for q in layered_util.layer_plans(csr, [(1, es, 0, 1, ITERS, 8) for es in (0, 1)])] == \
        ["bp_layer_kernel<8,lds>"] * 2
    return _layered_jobs(torch, "r36_600", False, seed, first, want)


def _job_layered_q(torch, seed, first, want):
    from tests import layered_q_util, layered_util
    csr = layered_util.graph_csr("r36_602")
    assert [q["name"] for q in layered_q_util.layer_q_plans(csr, [(1, es, 0, 1, ITERS, 8) for es in (0, 1)])] == \
        ["bp_layer_q_kernel<8>"] * 2
    return _layered_jobs(torch, "r36_602", True, seed, first, want)


def _job_sample_regular(case):
    def make(torch, seed, first, want):
        from iib_project_ldpc_codes_amd import _native
        c = u.BY_NAME[case]
        n, dv, dc, G = c["n"], c["dv"], c["dc"], c["B"]
        E = n * dv
        assert (E >= u.SEQ_E) == ("seq" in case)  # the sequential-draw sampler resets its search control per launch
        w = u.expected(c, u.true_indices(first, G), seed) if want else (None,) * 3
        j = su.Job(torch, case)
        chk = j.output((G, E), torch.int32, w[0], "check_lookup")
        var = j.output((G, E), torch.int32, w[1], "variable_lookup")
        att = j.output((G,), torch.int32, w[2], "attempts")
        j.call(lambda s: _native.check(_native.lib().ldpc_sample_regular_dev(
            n, dv, dc, seed, first, G, chk.data_ptr(), var.data_ptr(), att.data_ptr(), j.stream_ptr(s)),
            "ldpc_sample_regular_dev"))
        return [j]
    return make


def _job_sample_csr(torch, seed, first, want):
    from iib_project_ldpc_codes_amd import _native
    c = u.BY_NAME["sample-csr-2000"]
    vptr, cptr = [np.ascontiguousarray(a, np.int32) for a in u.csr_ptrs(c["n"])]
    E, G = int(vptr[-1]), c["B"]
    w = u.expected(c, u.true_indices(first, G), seed) if want else (None,) * 3
    j = su.Job(torch, "sample-csr-2000")
    cv = j.output((G, E), torch.int32, w[0], "check_var")
    vs = j.output((G, E), torch.int32, w[1], "var_slot")
    att = j.output((G,), torch.int32, w[2], "attempts")
    j.call(lambda s: _native.check(_native.lib().ldpc_sample_csr_dev(
        c["n"], len(cptr) - 1, vptr.ctypes.data, cptr.ctypes.data, seed, first, G, cv.data_ptr(), vs.data_ptr(),
        att.data_ptr(), j.stream_ptr(s)), "ldpc_sample_csr_dev"))
    return [j]


def _job_ensemble_decode(torch, seed, first, want):
    """The graphs are sampled in the same queue, in front of the two decodes that read them"""
    from iib_project_ldpc_codes_amd import _native, decoder
    from tests.test_ens_plan import ens_plans
    n, dv, dc, B = 200, 3, 6, 8
    rc, plans = ens_plans(n, dv, dc, [(1, es, 0, 1, ITERS, B) for es in (0, 1)])
    assert rc == 0 and [q["name"] for q in plans] == ["bp_ens_kernel<8,lds>"] * 2
    idx = u.true_indices(first, B)
    llr_h = u.channel_rows(oracle.CH_BSC, 0.04, seed, idx, n)
    j = su.Job(torch, "ensemble decode")
    if want:
        chk_h, var_h, _ = u.regular_graphs(n, dv, dc, seed, idx)
    chk = j.output((B, n * dv), torch.int32, chk_h if want else None, "check_lookup")
    var = j.output((B, n * dv), torch.int32, var_h if want else None, "variable_lookup")
    llr = j.late_input(llr_h)
    j.call(lambda s: _native.check(_native.lib().ldpc_sample_regular_dev(
        n, dv, dc, seed, first, B, chk.data_ptr(), var.data_ptr(), None, j.stream_ptr(s)), "ldpc_sample_regular_dev"))
    for es in (False, True):
        w = (None,) * 3
        if want:
            rows = [oracle.bp_decode_batch(oracle.csr_from_lists(var_h[b], chk_h[b], n, n * dv // dc, dv, dc),
                                           llr_h[b:b + 1], ITERS, 1, alpha=ALPHA, early_stop=es) for b in range(B)]
            w = [np.concatenate([r[k] for r in rows]) for k in range(3)]
        post = j.output((B, n), torch.float32, w[0], "post es=%d" % es)
        hard = j.output((B, n), torch.uint8, w[1], "hard es=%d" % es)
        its = j.output((B,), torch.int32, w[2], "its es=%d" % es)
        j.call(lambda s, es=es, post=post, hard=hard, its=its: decoder.bp_ensemble_decode_dev(
            n, dv, dc, chk, var, llr, ITERS, "minsum", ALPHA, es, post=post, hard=hard, its=its, stream=s))
    return [j]


def _job_ml(ens):
    def make(torch, seed, first, want):
        from iib_project_ldpc_codes_amd import decoder
        n, B = (100, 16) if ens else (200, 16)
        m = n // 2
        idx = u.true_indices(first, B)
        words = u.channel_rows(oracle.CH_BEC, ML_DECODE_EPS, seed, idx, n).astype(np.uint8)
        j = su.Job(torch, "ml ens=%d" % ens)
        dw = j.late_input(words)
        if ens:
            chk_h = u.regular_graphs(n, 3, 6, seed, idx)[0]
            chk = j.late_input(chk_h)
            cptr = np.arange(m + 1, dtype=np.int32) * 6
            rows = [oracle.ml_decode_batch(cptr, chk_h[b], words[b], n, m) for b in range(B)] if want else None
            w = [np.concatenate([r[k] for r in rows]) for k in range(2)] if want else (None, None)
        else:
            g, csr, _ = su.graph(("reg", n, 9))
            w = oracle.ml_decode_batch(csr[0], csr[1], words, n, m) if want else (None, None)
        out = j.output((B, n), torch.uint8, w[0], "out")
        uns = j.output((B,), torch.int32, w[1], "unsolved")
        if want:
            assert (w[1] > 0).any() and (w[1] == 0).any()
        if ens:
            j.call(lambda s: decoder.ml_ensemble_decode_dev(n, 3, 6, chk, dw, out=out, unsolved=uns, stream=s))
        else:
            j.call(lambda s: decoder.ml_decode_dev(g, dw, out=out, unsolved=uns, stream=s))
        return [j]
    return make


def _mc_job(torch, name, mc, want, first, B, want_ml=None, stop=0):
    """A Monte-Carlo batch of `mc` into garbage counters that are zeroed behind the stall"""
    j = su.Job(torch, name)
    if want_ml is None:
        mc.counters = j.accumulator((len(mc.counters),), torch.int64, want, "counters")
    else:  # index64_util._ml_counters: [trials, MP frame, MP bit, ML frame, ML bit | MP curve]
        mc.counters = j.accumulator((len(mc.counters),), torch.int64, None)
        mc.counters_ml = j.accumulator((len(mc.counters_ml),), torch.int64, None)

        def check(mp_t=mc.counters, ml_t=mc.counters_ml):
            a, b = mp_t.cpu().numpy(), ml_t.cpu().numpy()
            assert b[0] == B and b[3] == 0 and b[2] == b[4], b
            np.testing.assert_array_equal(np.concatenate([a[:3], b[1:3], a[4:]]), want, err_msg=name)
        j.extra = check if want is not None else None
    j.call(lambda s: mc.run_batch(first, B, stop, stream=s))
    return j


def _job_mc(case, B=None):
    """ldpc_mc_*_batch_dev of an index64_util case (a soft case: fixed count and early stop)"""
    def make(torch, seed, first, want):
        from iib_project_ldpc_codes_amd.decoder import Quant
        from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
        from tests import layered_q_util, layered_util
        from tests.test_ens_plan import ens_plans
        c = dict(u.BY_NAME[case], B=B or u.BY_NAME[case]["B"])
        fam, nB = c["family"], c["B"]
        w = u.expected(c, u.true_indices(first, nB), seed) if want else None
        kw = dict(seed=seed, batch=nB)
        if fam == "bec":
            # with a stop two frame errors behind trial 20, so the cutoff kernel's read of the trial
            # rows is held to the stream as well (without a stop it writes B whatever it reads)
            n = c["n"]
            assert bec_plans(n, n // 2, [(BEC_MC, nB, u.BEC_ITERS)])[0]["name"] == c["kernel"]
            stop = 1
            if want:
                w, stop = u.expected(dict(c, name=case + "-stop", stop_after=(20, 2)), u.true_indices(first, nB), seed)
                stop = int(stop[0])
                assert w[1] == stop > 0 and 21 < w[0] < nB, w[:2]
            mc = MonteCarlo(su.graph(("reg", n, 11))[0], "bec", u.EPS, u.BEC_ITERS, expurgation=-1, **kw)
            return [_mc_job(torch, case, mc, w, first, nB, stop=stop)]
        if fam == "bec_ens":
            n = c["n"]
            assert bec_plans(n, n // 2, [(BEC_ENS_MC, nB, u.BEC_ITERS)])[0]["name"] == c["kernel"]
            mc = MonteCarlo.ensemble(n, 3, 6, "bec", u.EPS, u.BEC_ITERS, expurgation=-1, **kw)
            return [_mc_job(torch, case, mc, w and u.counters(*w), first, nB)]
        if fam == "ml":
            kw.update(optimal=True, message_passing=True)
            if c["ens"]:
                mc = MonteCarlo.ensemble(c["n"], 3, 6, "bec", u.ML_EPS, u.ML_ITERS, **kw)
            else:
                mc = MonteCarlo(su.graph(("reg", c["n"], 9))[0], "bec", u.ML_EPS, u.ML_ITERS, **kw)
            return [_mc_job(torch, case, mc, w and w[0], first, nB, want_ml=True)]
        jobs = []
        for k, es in enumerate(u.MODES):
            soft = dict(algo="minsum", alpha=ALPHA, early_stop=es, **kw)
            if fam == "soft":
                g, csr, env = su.graph(c["graph"], c["noloc"])
                assert _plan_names(csr, [(1, int(es), 1, 0, ITERS, nB)], env) == [c["kernel"]]
                mc = MonteCarlo(g, "bsc", c["p"], ITERS, **soft)
            elif fam == "soft_ens":
                rc, plans = ens_plans(*c["shape"], [(1, int(es), 1, 0, ITERS, nB)])
                assert rc == 0 and plans[0]["name"] == c["kernel"]
                mc = MonteCarlo.ensemble(*c["shape"], "bsc", c["p"], ITERS, **soft)
            elif fam == "layer":
                csr = layered_util.graph_csr(c["graph"])
                assert layered_util.layer_plans(csr, [(1, int(es), 1, 0, ITERS, nB)])[0]["name"] == c["kernel"]
                mc = MonteCarlo(layered_util.graph(c["graph"]), "bsc", c["p"], ITERS, schedule="layered", **soft)
            else:
                assert fam == "layer_q"
                csr = layered_util.graph_csr(c["graph"])
                assert layered_q_util.layer_q_plans(csr, [(1, int(es), 1, 0, ITERS, nB)])[0]["name"] == c["kernel"]
                mc = MonteCarlo(layered_util.graph(c["graph"]), "bsc", c["p"], ITERS, schedule="layered",
                                quant=Quant(*u.QUANT), **soft)
            jobs.append(_mc_job(torch, "%s es=%d" % (case, es), mc, w and w[k], first, nB))
        return jobs
    return make


# entry -> (jobs of one call sequence, how the stream is passed)
LATE = {
    "channel": (_job_channel, "arg"),
    "bec_decode-8": (_job_bec_decode(8, "bec_kernel<256>"), "current"),
    "bec_decode-128": (_job_bec_decode(128, "bec_dec_bits_kernel<256,1,u32>"), "arg"),
    "bp_decode-loc-10000": (_job_flood(REG10K, False, "bp_loc_kernel", P10K, persistent=True), "arg"),
    "bp_decode-lds-1000": (_job_flood(REG1K, False, "bp_lds_kernel<3,6>", P1K), "current"),
    "bp_decode-lds-1000-noloc": (_job_flood(REG1K, True, "bp_lds_kernel<3,6>", P1K), "arg"),
    "bp_decode-irr-r48_9216": (_job_flood(("fb", "r48_9216"), False, "bp_irr_kernel<lds+slab>", 0.04), "current"),
    "bp_decode-generic-r58_320": (_job_flood(("fb", "r58_320"), False, "bp_generic_kernel<8,lds>", 0.04), "arg"),
    "bp_decode-generic-r58_8800": (_job_flood(("fb", "r58_8800"), False, "bp_generic_kernel<8,gmem>", 0.05), "current"),
    "layered": (_job_layered, "arg"),
    "layered_q": (_job_layered_q, "current"),
    "sample_regular-1000": (_job_sample_regular("sample-reg-1000-3-6"), "arg"),
    "sample_regular-seq-2732": (_job_sample_regular("sample-seq-2732"), "current"),
    "sample_csr": (_job_sample_csr, "arg"),
    "ensemble_decode": (_job_ensemble_decode, "current"),
    "ml_decode": (_job_ml(False), "arg"),
    "ml_ensemble_decode": (_job_ml(True), "current"),
    "mc-bec": (_job_mc("bec-bits-96-40"), "arg"),
    "mc-lds-1000": (_job_mc("soft-ms-1000"), "current"),
    "mc-loc-10000": (_job_mc("soft-loc-10000"), "arg"),
    "mc-irr-r48_9216": (_job_mc("soft-irr-r48_9216"), "current"),
    "mc-generic-r58_8800": (_job_mc("soft-generic-r58_8800", B=8), "arg"),
    "mc_layered": (_job_mc("layer-r36_600"), "current"),
    "mc_layered_q": (_job_mc("layerq-r36_602"), "arg"),
    "mc_ensemble-bec": (_job_mc("bec-ens-96-40"), "current"),
    "mc_ensemble_soft": (_job_mc("ens-200-3-6"), "arg"),
    "mc_ml-fixed": (_job_mc("ml-fixed-200"), "current"),
    "mc_ml-ensemble": (_job_mc("ml-ens-100"), "arg"),
}


def _check(jobs):
    for j in jobs:
        j.check()
        if getattr(j, "extra", None):
            j.extra()


@pytest.mark.parametrize("entry", sorted(LATE))
def test_late_inputs(torch, entry):
    """Behind the stall on a side stream: the real inputs copied over zero-filled ones (Monte-Carlo:
    garbage counters zeroed), the outputs filled with the sentinel, then the entry.  A kernel, memset
    or copy of the entry that runs on another stream works on the stale data."""
    make, how = LATE[entry]
    S = su.side_streams(torch)[0]
    su.run_jobs(torch, make(torch, WARM_SEED, WARM_FIRST, False), S, how, stalled=False)  # the warm-up
    jobs = make(torch, SEED, FIRST, True)
    ended = su.run_jobs(torch, jobs, S, how)
    if entry not in BLOCKING:
        assert not ended, "the call blocked the host until the stall had ended (or the stall is too short)"
    _check(jobs)


# ---------------------------------------------------------- 2. queued calls on one stream
def _stop_inside_second_batch(curve, B, X=-1):
    """(stop, frame errors of batch 1) with the cut strictly inside the second of three batches of B"""
    f = np.asarray(curve)[:, -1]
    fe = (f > X) & (f != 0)
    first, inside = int(fe[:B].sum()), np.nonzero(fe[B:2 * B - 1])[0]
    assert inside.size, "no frame error inside batch 2: pick other parameters"
    return first + 1, first


def test_queued_calls_on_one_stream(torch):
    """Ten calls behind one stall, no host synchronisation between them: two early-stop decodes with
    posteriors on the persistent grid (its codeword counter is zeroed per launch, on the stream;
    n = 10,000) and two at n = 1,000, a 50-iteration Monte-Carlo batch of 512 and a 5-iteration one of
    64 through the same trial buffer, and two trios of equal batches into one counters tensor each
    whose stop falls inside the second batch."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    S = su.side_streams(torch)[0]
    csr10k = u.fixed_graph(REG10K)[1]
    plan = bp_plans(csr10k, [(1, 1, 0, 1, ITERS, 600)])[0]
    assert plan["name"] == "bp_loc_kernel" and plan["persistent"] == 1 and 0 < plan["slab"] == plan["counter"], plan
    csr1k = u.fixed_graph(REG1K)[1]
    assert _plan_names(csr1k, [(1, 1, 0, 1, ITERS, 600), (1, 1, 1, 0, 50, 512), (1, 1, 1, 0, ITERS, 64),
                               (1, 1, 1, 0, ITERS, 16)]) == ["bp_lds_kernel<3,6>"] * 4
    nb, Bb, Bs = 96, 40, 16
    assert bec_plans(nb, nb // 2, [(BEC_MC, Bb, u.BEC_ITERS)])[0]["name"] == "bec_mc_bits_kernel<256,1,u32>"

    def bec_trio(seed, first, want):
        g = su.graph(("reg", nb, 11))[0]
        j = su.Job(torch, "bec trio")
        w, stop = None, 1
        if want:
            words = u.channel_rows(oracle.CH_BEC, u.EPS, seed, u.true_indices(first, 3 * Bb), nb)
            curve, its = u._bec_curves(words, u.BEC_ITERS, g)
            stop, f1 = _stop_inside_second_batch(curve, Bb)
            w = u.counters(curve, its, -1, stop)
            assert f1 < stop == w[1] and Bb < w[0] < 2 * Bb, (f1, stop, w[:2])
            np.testing.assert_array_equal(w, u.counters(curve[:2 * Bb], its[:2 * Bb], -1, stop))  # batch 3 adds nothing
        mc = MonteCarlo(g, "bec", u.EPS, u.BEC_ITERS, expurgation=-1, seed=seed, batch=Bb)
        mc.counters = j.accumulator((len(mc.counters),), torch.int64, w, "counters")
        for k in range(3):
            j.call(lambda s, k=k: mc.run_batch(first + k * Bb, Bb, stop, stream=s))
        return j

    def soft_trio(seed, first, want):
        stop = 1
        if want:
            parts = [su.minsum_trials(REG1K, 0.05, seed, first + k * Bs, Bs, ITERS, True) for k in range(3)]
            curve, its = np.concatenate([c for c, _ in parts]), np.concatenate([i for _, i in parts])
            stop, f1 = _stop_inside_second_batch(curve, Bs)
            w = u.counters(curve, its, -1, stop)
            assert f1 < stop == w[1] and Bs < w[0] < 2 * Bs, (f1, stop, w[:2])
        return su.mc_job(torch, REG1K, 0.05, seed, [(first + k * Bs, Bs) for k in range(3)], ITERS, True, stop,
                         want=want, name="min-sum trio")

    def sequence(seed, first, want):
        return [su.decode_job(torch, REG10K, P10K, seed, first, 600, ITERS, True, want=want, name="loc A"),
                su.decode_job(torch, REG10K, P10K, seed + 1, first + 7000, 600, ITERS, True, want=want, name="loc B"),
                su.decode_job(torch, REG1K, P1K, seed, first, 600, ITERS, True, want=want, name="lds A"),
                su.decode_job(torch, REG1K, P1K, seed + 1, first + 7000, 600, ITERS, True, want=want, name="lds B"),
                su.mc_job(torch, REG1K, P1K, seed, [(first, 512)], 50, True, want=want),
                su.mc_job(torch, REG1K, P1K, seed + 2, [(first + 512, 64)], ITERS, True, want=want),
                bec_trio(seed, first, want), soft_trio(seed, first, want)]

    su.run_jobs(torch, sequence(WARM_SEED, WARM_FIRST, False), S, "arg", stalled=False)
    jobs = sequence(SEED, FIRST, True)
    assert not su.run_jobs(torch, jobs, S, "arg"), "a queued call blocked the host (or the stall is too short)"
    _check(jobs)


# --------------------------------------------------------- 4. growth between queued calls
def test_growth_between_queued_calls(torch):
    """Small, large, small on the second side stream, which no earlier test of this file has used, with
    no host synchronisation in between: the large calls grow the trial rows, and the slabs of the
    n = 8,800 decode, by freeing them, which synchronises the device.  No stall
    here on purpose: growth relies on that synchronisation, and this test must not become a
    use-after-free probe if that ever changes."""
    S = su.side_streams(torch)[1]
    slab = ("fb", "r58_8800")
    plans = bp_plans(u.fixed_graph(slab)[1], [(1, 1, 0, 1, ITERS, 8), (1, 1, 0, 1, ITERS, 64)])
    assert [q["name"] for q in plans] == ["bp_generic_kernel<8,gmem>"] * 2 and plans[0]["scratch"] < plans[1]["scratch"]
    jobs = [su.mc_job(torch, REG1K, P1K, SEED, [(FIRST, 8)], ITERS, True),
            su.decode_job(torch, slab, 0.05, SEED, FIRST, 8, ITERS, True),
            su.mc_job(torch, REG1K, P1K, SEED + 1, [(FIRST + 100, 2048)], 20, True),
            su.decode_job(torch, slab, 0.05, SEED + 1, FIRST + 100, 64, ITERS, True),
            su.mc_job(torch, REG1K, P1K, SEED + 2, [(FIRST + 5000, 8)], ITERS, True),
            su.decode_job(torch, slab, 0.05, SEED + 2, FIRST + 5000, 8, ITERS, True)]
    su.run_jobs(torch, jobs, S, "arg", stalled=False)
    _check(jobs)


# ------------------------------------------------- 3. two streams and the default stream
def test_two_streams_and_the_default_stream(torch):
    """Both side streams and the default stream wait for one stall and then work at once on the same
    graph and shapes, each with its own seed: a min-sum Monte-Carlo batch of 16,384 (50 iterations)
    and an early-stop decode with posteriors; each result equals its own oracle, so no two streams
    were handed the same trial rows.  The host form, on the workspace of the NULL stream, is right
    as well while the side streams have work queued."""
    from iib_project_ldpc_codes_amd import _native
    S1, S2 = su.side_streams(torch)
    D = torch.cuda.default_stream()
    B, iters = 16384, 50
    assert _plan_names(u.fixed_graph(REG1K)[1], [(1, 1, 1, 0, iters, B), (1, 1, 0, 1, ITERS, 600)]) == \
        ["bp_lds_kernel<3,6>"] * 2

    def pair(k, seed, first, want):
        p = 0.05 if k == 0 else P1K  # 0.05: a few trials of the 16,384 still fail after 50 iterations
        return [su.mc_job(torch, REG1K, p, seed + 10 * k, [(first + k * B, B)], iters, True, want=want),
                su.decode_job(torch, REG1K, P1K, seed + 10 * k, first + 9000 * k, 600, ITERS, True, want=want)]

    streams = (S1, S2, D)
    for k, s in enumerate(streams):  # the warm-up, stream by stream
        su.run_jobs(torch, pair(k, WARM_SEED, WARM_FIRST, False), s, "arg", stalled=False)
    jobs = [pair(k, SEED, FIRST, True) for k in range(3)]
    for js in jobs:
        for j in js:
            j.fill()
    torch.cuda.synchronize()
    done = su.stall(torch, S1)
    S2.wait_event(done)
    D.wait_event(done)
    for s, js in zip(streams, jobs):
        with torch.cuda.stream(s):
            for j in js:
                j.late()
    for s, js in zip(streams, jobs):  # interleaved: Monte-Carlo on every stream, then the decodes
        js[0].enqueue(s)
    for s, js in zip(streams, jobs):
        js[1].enqueue(s)
    assert not done.query(), "a call blocked the host (or the stall is too short)"
    # the host form while the side streams have work queued
    g = su.graph(REG1K)[0]
    v2c, c2v = np.ascontiguousarray(g.variable_lookup, np.int32), np.ascontiguousarray(g.check_lookup, np.int32)
    Bh = 24
    llr = np.ascontiguousarray(su.bsc_llr(REG1K, P1K, SEED + 99, FIRST, Bh))
    post, hard, its = np.full((Bh, g.n), np.nan, np.float32), np.full((Bh, g.n), 0x7F, np.uint8), np.full(Bh, -1, np.int32)
    rc = _native.lib().ldpc_bp_decode_batch(v2c.ctypes.data, c2v.ctypes.data, g.n, g.k, 3, 6, llr.ctypes.data, Bh, ITERS,
                                            1, ALPHA, 1, post.ctypes.data, hard.ctypes.data, its.ctypes.data)
    _native.check(rc, "ldpc_bp_decode_batch")
    for s in streams:
        s.synchronize()
    for got, w in zip((post, hard, its), su.minsum_decode(REG1K, P1K, SEED + 99, FIRST, Bh, ITERS, True)):
        np.testing.assert_array_equal(got, w, err_msg="host form")
    for js in jobs:
        _check(js)


# -------------------------------------------------------------------- 5. two host threads
def test_two_host_threads(torch):
    """Two threads, a stream each, ten calls each, a decode entry and a Monte-Carlo entry in turn
    (decode_entry takes g_mu and the workspace's lock, mc_entry the workspace's alone): all twenty
    results equal the oracle, and an invalid call in one thread leaves the other thread's
    ldpc_last_error() as it was."""
    from iib_project_ldpc_codes_amd import _native
    L = _native.lib()
    streams = su.side_streams(torch)
    for k, s in enumerate(streams):  # the warm-up: workspaces grown, kernels loaded
        su.run_jobs(torch, [su.mc_job(torch, REG1K, P1K, WARM_SEED, [(WARM_FIRST, 8)], ITERS, True, want=False),
                            su.decode_job(torch, REG1K, P1K, WARM_SEED, WARM_FIRST, 8, ITERS, True, want=False)], s,
                    "arg", stalled=False)
    jobs = []
    for k in range(2):
        js = []
        for i in range(5):
            first = FIRST + 1000 * k + 8 * i
            js.append(su.decode_job(torch, REG1K, P1K, SEED + k, first, 8, ITERS, True, name="thread %d" % k))
            js.append(su.mc_job(torch, REG1K, P1K, SEED + k, [(first, 8)], ITERS, bool(i & 1), name="thread %d" % k))
        for j in js:
            j.fill()
        jobs.append(js)
    torch.cuda.synchronize()
    barrier = threading.Barrier(2, timeout=30)
    errors, failed = [None, None], []
    g = su.graph(REG1K)[0].handle()

    def work(k):
        try:
            torch.cuda.set_device(0)
            s = streams[k]
            with torch.cuda.stream(s):
                for j in jobs[k]:
                    j.late()
            # thread 1 fails a call of its own first; thread 0 then fails another one in between
            if k == 1:
                assert L.ldpc_bp_decode_batch_dev(g, None, 0, ITERS, 2, ALPHA, 1, None, None, None, None) == -1
                assert "algo must be" in _native.last_error()
            barrier.wait()
            for i, j in enumerate(jobs[k]):
                j.enqueue(s)
                if k == 0 and i == 4:
                    assert L.ldpc_mc_batch_dev(g, 1, 0.04, 1, 0, -1, ITERS, 1, ALPHA, 1, -1, 0, None, None) == -1
                    assert "bad MC arguments" in _native.last_error()
            barrier.wait()
            errors[k] = _native.last_error()
            s.synchronize()
        except BaseException as e:  # noqa: B036 -- reported by the main thread
            failed.append((k, repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a thread has not returned"
    assert not failed, failed
    assert "bad MC arguments" in errors[0] and "algo must be" in errors[1], errors
    for js in jobs:
        _check(js)


# ------------------------------------------------------------------------- 6. two devices
def test_two_devices_null_stream(torch):
    """The same call on the default streams of devices 0 and 1, both queued before either is read:
    the workspace key holds the device."""
    from iib_project_ldpc_codes_amd import _native
    if _native.lib().ldpc_device_count() < 2:
        pytest.skip("needs two devices")
    assert _plan_names(u.fixed_graph(REG1K)[1], [(1, 1, 1, 0, ITERS, 64), (1, 1, 0, 1, ITERS, 64)]) == \
        ["bp_lds_kernel<3,6>"] * 2
    jobs = []
    try:
        for dev in (0, 1):
            torch.cuda.set_device(dev)
            D = torch.cuda.default_stream()
            su.run_jobs(torch, [su.mc_job(torch, REG1K, P1K, WARM_SEED, [(WARM_FIRST, 64)], ITERS, True, want=False),
                                su.decode_job(torch, REG1K, P1K, WARM_SEED, WARM_FIRST, 64, ITERS, True, want=False)],
                        D, "arg", stalled=False)
        for dev in (0, 1):
            torch.cuda.set_device(dev)
            js = [su.mc_job(torch, REG1K, P1K, SEED + dev, [(FIRST, 64)], ITERS, True),
                  su.decode_job(torch, REG1K, P1K, SEED + dev, FIRST, 64, ITERS, True)]
            for j in js:
                j.fill()
                j.late()
            torch.cuda.synchronize()
            jobs.append(js)
        for dev in (0, 1):
            torch.cuda.set_device(dev)
            for j in jobs[dev]:
                j.enqueue(None)
        for dev in (0, 1):
            torch.cuda.set_device(dev)
            torch.cuda.synchronize()
            _check(jobs[dev])
    finally:
        torch.cuda.set_device(0)
