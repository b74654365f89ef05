"""Gallager A/B on the device (csrc/gb.hip through ldpc_gb_decode_batch_dev, ldpc_mc_gb_batch_dev and
MonteCarlo(algo="gallager")) against tests/gallager_ref.py.  Everything is an integer: every comparison
is bit for bit.

Received words are the oracle's BSC stream (1 where its LLR is negative) under seed 11 from trial 0.
Every early-stop decode at the 20- (or 50-) iteration cap and every Monte-Carlo case first asserts, on the
reference alone, that at least 8 of its frames stop before the cap and at least 8 run to it
(gallager_util.P_MIX: how the crossover probabilities were chosen); at 0, 1 or 3 iterations no frame can
do both, those are the same words cut short.
"""
import numpy as np
import pytest

from tests import gallager_util as gu
from tests import gallager_ref as ref

pytestmark = pytest.mark.gpu

SEED = gu.SEED
GRAPHS = ("r36_600", "r36_602", "r48_256", "r510_640", "mixA", "mixB")
BATCH = 264
ITERS = (0, 1, 3, 20)
CASES = [(name, b) for name in GRAPHS for b in gu.b_values(name)]
# Every plane shape the plan gives a (3,6) graph, at the smallest n that reaches it (tests/test_gb_plan.py
# has the sizes): (graph, crossover probability of its 40-frame early-stop case, kernel of a plain decode,
# kernel under early stop)
SHAPES = [("r36_2052", 0.037, "gb_kernel<1024,u32>", "gb_kernel<1024,u32,es>"),
          ("r36_8000", 0.039, "gb_kernel<1024,u32>", "gb_kernel<1024,u16,es>"),
          ("r36_16000", 0.039, "gb_kernel<1024,u16>", "gb_kernel<1024,u8,es>"),
          ("r36_20002", 0.039, "gb_kernel<1024,u8>", None)]  # the plain decode alone: r36_16000 has u8 with X
SHAPE_B, SHAPE_ITERS = 40, 50
# Monte-Carlo cases: b = 0 everywhere and the issue's rows with another b
MC_CASES = [(name, 0) for name in GRAPHS] + [("r48_256", 2), ("r510_640", 3), ("mixA", 2)]


def _batches(cw):
    return (1, cw - 1, cw + 1, BATCH)


def plan_calls():
    """(graph, B, iters, early_stop, mc) of every device call of this file (tests/test_gb_plan.py holds the
    plan to its invariants on them)."""
    calls = []
    for name, _ in CASES:
        calls += [(name, B, it, es, 0) for es in (0, 1) for it in ITERS for B in _batches(32)]
    for name, _, _, es_kernel in SHAPES:
        calls.append((name, 9, 3, 0, 0))
        if es_kernel:
            calls += [(name, SHAPE_B, SHAPE_ITERS, 1, 0), (name, SHAPE_B, SHAPE_ITERS, 1, 1), (name, 9, 3, 0, 1)]
    calls += [("r36_10000", 64, 50, 1, 0)]
    for name, _ in MC_CASES:
        calls += [(name, 200, 20, 1, 1), (name, 64, 20, 1, 1), (name, BATCH, 20, 1, 1), (name, BATCH, 20, 0, 1)]
    calls += [("r36_602", 8, 20, 1, 1), ("r36_600", 100, 20, 1, 1), ("r36_602", 33, 20, 1, 0), ("r48_256", 70, 3, 0, 0)]
    return calls


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


def _decode(torch, name, Y, iters, b, es, **kw):
    from iib_project_ldpc_codes_amd import decoder
    hard, its = decoder.gallager_decode_dev(gu.graph(name), torch.from_numpy(np.array(Y)).cuda(), iters, b,
                                            es, **kw)
    torch.cuda.synchronize()
    return (None if hard is None else hard.cpu().numpy()), (None if its is None else its.cpu().numpy())


def _mc(torch, name, p, iters, b, es, batches, X=-1, stop=0, seed=SEED):
    """The counters after the batches [(first, B), ...] queued into one counters tensor."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    mc = MonteCarlo(gu.graph(name), "bsc", p, iters, algo="gallager", flip_threshold=b, early_stop=es, expurgation=X,
                    seed=seed, batch=max(B for _, B in batches))
    for first, B in batches:
        mc.run_batch(first, B, stop)
    torch.cuda.synchronize()
    return mc.counters.cpu().numpy()


@pytest.mark.parametrize("name,b", CASES)
def test_decode_bit_exact(torch, name, b):
    """b in {0, 1, 2, dv - 1}, early stop on and off, 0 / 1 / 3 / 20 iterations, B = 1, one short of a
    workgroup's codewords, one over, and 264 (nine workgroups): hard decisions and iteration counts."""
    p = gu.P_MIX[(name, b)]
    cw = gu.plan(name, BATCH, 20, True, False)["cw_per_wg"]
    assert cw == gu.plan(name, BATCH, 20, False, False)["cw_per_wg"] == 32
    Y = gu.bsc_bits(name, p, SEED, 0, BATCH)
    for es in (False, True):
        for iters in ITERS:
            hard, its, _ = gu.decoded(name, p, SEED, 0, BATCH, iters, b, es)
            if es and iters == 20:
                gu.assert_stop_mix(its, 20)
            for B in _batches(cw):  # words decode on their own: the first B rows of the reference
                h, i = _decode(torch, name, Y[:B], iters, b, es)
                np.testing.assert_array_equal(h, hard[:B], err_msg="hard es=%d iters=%d B=%d" % (es, iters, B))
                np.testing.assert_array_equal(i, its[:B], err_msg="its es=%d iters=%d B=%d" % (es, iters, B))


@pytest.mark.parametrize("name", GRAPHS)
def test_dense_words_and_high_bits(torch, name):
    """Words at p = 0.5 (nothing converges: every frame runs to the cap), and BSC words whose bytes carry
    random high bits (only bit 0 is read)."""
    n = gu.shape(name)[0]
    rng = np.random.default_rng(3)
    dense = (rng.random((33, n)) < 0.5).astype(np.uint8)
    hard, its, _ = ref.decode(gu.graph_csr(name), dense, 20, 0, True)
    assert (its == 20).all()
    h, i = _decode(torch, name, dense, 20, 0, True)
    np.testing.assert_array_equal(h, hard)
    np.testing.assert_array_equal(i, its)
    p = gu.P_MIX[(name, 0)]
    Y = gu.bsc_bits(name, p, SEED, 0, BATCH)[:33]
    hard, its, _ = gu.decoded(name, p, SEED, 0, BATCH, 20, 0, True)
    h, i = _decode(torch, name, Y | (rng.integers(0, 128, Y.shape, dtype=np.uint8) << 1), 20, 0, True)
    np.testing.assert_array_equal(h, hard[:33])
    np.testing.assert_array_equal(i, its[:33])


def test_null_outputs(torch):
    """d_hard and d_its NULL in turn: the other is written as ever."""
    name, b = "r36_602", 0
    p = gu.P_MIX[(name, b)]
    Y = gu.bsc_bits(name, p, SEED, 0, BATCH)[:33]
    hard, its, _ = gu.decoded(name, p, SEED, 0, BATCH, 20, b, True)
    h, i = _decode(torch, name, Y, 20, b, True, want_hard=False)
    assert h is None
    np.testing.assert_array_equal(i, its[:33])
    h, i = _decode(torch, name, Y, 20, b, True, want_its=False)
    assert i is None
    np.testing.assert_array_equal(h, hard[:33])


@pytest.mark.parametrize("name,p,plain,stopping", SHAPES)
def test_every_plane_shape(torch, name, p, plain, stopping):
    """The plan first, then bit for bit: a plain decode of 9 words (two workgroups at any plane word), and
    where the planes fit with X the 40-frame early-stop decode and the same trials as a Monte-Carlo batch
    with and without early stop."""
    assert gu.plan(name, 9, 3, False, False)["name"] == plain
    Y = gu.bsc_bits(name, p, SEED, 0, SHAPE_B)
    hard, its, _ = ref.decode(gu.graph_csr(name), Y[:9], 3, 0, False)
    h, i = _decode(torch, name, Y[:9], 3, 0, False)
    np.testing.assert_array_equal(h, hard)
    np.testing.assert_array_equal(i, its)
    if stopping is None:
        return
    assert gu.plan(name, SHAPE_B, SHAPE_ITERS, True, False)["name"] == stopping
    assert gu.plan(name, SHAPE_B, SHAPE_ITERS, True, True)["name"] == stopping[:-1] + ",mc>"
    hard, its, curve = gu.decoded(name, p, SEED, 0, SHAPE_B, SHAPE_ITERS, 0, True)
    gu.assert_stop_mix(its, SHAPE_ITERS)
    h, i = _decode(torch, name, Y, SHAPE_ITERS, 0, True)
    np.testing.assert_array_equal(h, hard)
    np.testing.assert_array_equal(i, its)
    np.testing.assert_array_equal(_mc(torch, name, p, SHAPE_ITERS, 0, True, [(0, SHAPE_B)]), ref.mc_counters(curve, its))
    _, its3, curve3 = ref.decode(gu.graph_csr(name), Y[:9], 3, 0, False)
    assert gu.plan(name, 9, 3, False, True)["name"] == stopping.replace(",es>", ",mc>")
    np.testing.assert_array_equal(_mc(torch, name, p, 3, 0, False, [(0, 9)]), ref.mc_counters(curve3, its3))


def test_config2_shape(torch):
    """(3,6), n = 10,000, Gallager A at p = 0.038, 64 frames, at most 50 iterations with early stop: the
    16-bit plane word.  The reference alone has 49 frames stopping early and 15 at the cap."""
    name, p = "r36_10000", gu.P_MIX[("r36_10000", 0)]
    assert gu.plan(name, 64, 50, True, False)["name"] == "gb_kernel<1024,u16,es>"
    hard, its, _ = gu.decoded(name, p, SEED, 0, 64, 50, 0, True)
    assert gu.stop_mix(its, 50) == (49, 15)
    h, i = _decode(torch, name, gu.bsc_bits(name, p, SEED, 0, 64), 50, 0, True)
    np.testing.assert_array_equal(h, hard)
    np.testing.assert_array_equal(i, its)


@pytest.mark.parametrize("name,b", MC_CASES)
def test_mc_counters_and_curve(torch, name, b):
    """Two consecutive batches (200 + 64 trials) into one counters tensor, expurgation -1 and 2, a frame-
    error stop that cuts inside the batch, and a run without early stop: every counter and the curve."""
    p = gu.P_MIX[(name, b)]
    _, its, curve = gu.decoded(name, p, SEED, 0, BATCH, 20, b, True)
    gu.assert_stop_mix(its, 20)
    for X in (-1, 2):
        np.testing.assert_array_equal(_mc(torch, name, p, 20, b, True, [(0, 200), (200, 64)], X=X),
                                      ref.mc_counters(curve, its, X), err_msg="X=%d" % X)
    frames = int((curve[:, -1] != 0).sum())
    assert frames >= 8
    stop = frames // 2  # the cut lies inside the batch
    want = ref.mc_counters(curve, its, -1, stop)
    assert 0 < want[0] < BATCH and want[1] == stop
    np.testing.assert_array_equal(_mc(torch, name, p, 20, b, True, [(0, BATCH)], stop=stop), want)
    _, its_n, curve_n = gu.decoded(name, p, SEED, 0, BATCH, 20, b, False)
    assert (its_n == 20).all()
    np.testing.assert_array_equal(_mc(torch, name, p, 20, b, False, [(0, BATCH)]), ref.mc_counters(curve_n, its_n))


def test_mc_batch_across_2_to_the_32(torch):
    """first_cw = 2^32 - 3, B = 8 under a seed with a high word: trial index and seed in full 64-bit width."""
    from tests import index64_util as u
    name, b, p = "r36_602", 0, 0.03
    seed, first = u.SEED, u.T - 3
    _, its, curve = gu.decoded(name, p, seed, first, 8, 20, b, True)
    np.testing.assert_array_equal(_mc(torch, name, p, 20, b, True, [(first, 8)], seed=seed), ref.mc_counters(curve, its))
    for model, (idx, s) in u.wrong_index_models(first, 8, seed).items():  # the case tells the bug models apart
        y = (u.channel_rows(u.oracle.CH_BSC, p, s, idx, gu.shape(name)[0]) < 0).astype(np.uint8)
        assert (y != gu.bsc_bits(name, p, seed, first, 8)).any(), model


def test_queued_calls_on_a_side_stream(torch):
    """Two calls of different shapes (an early-stop decode of 33 words on r36_602, a plain 3-iteration
    decode of 70 words on r48_256) and a Monte-Carlo batch, queued on a side stream behind a stall with
    inputs that arrive late, no host synchronisation in between, one at the end."""
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    from tests import stream_util as su
    stream = su.side_streams(torch)[0]
    jobs = []
    for name, b, B, iters, es in (("r36_602", 0, 33, 20, True), ("r48_256", 2, 70, 3, False)):
        p = gu.P_MIX[(name, b)]
        hard, its, _ = gu.decoded(name, p, SEED, 0, BATCH, iters, b, es)
        j = su.Job(torch, "gallager decode %s" % name)
        bits = j.late_input(gu.bsc_bits(name, p, SEED, 0, BATCH)[:B])
        out_h = j.output((B, gu.shape(name)[0]), torch.uint8, hard[:B], "hard")
        out_i = j.output((B,), torch.int32, its[:B].astype(np.int32), "its")
        j.call(lambda s, g=gu.graph(name), bits=bits, iters=iters, b=b, es=es, h=out_h, i=out_i:
               decoder.gallager_decode_dev(g, bits, iters, b, es, hard=h, its=i, stream=s))
        jobs.append(j)
    name, b, p = "r36_600", 0, gu.P_MIX[("r36_600", 0)]
    _, its, curve = gu.decoded(name, p, SEED, 0, BATCH, 20, b, True)
    j = su.Job(torch, "gallager mc")
    mc = MonteCarlo(gu.graph(name), "bsc", p, 20, algo="gallager", early_stop=True, seed=SEED, batch=100)
    mc.counters = j.accumulator((len(mc.counters),), torch.int64, ref.mc_counters(curve[:200], its[:200]), "counters")
    for first in (0, 100):
        j.call(lambda s, first=first: mc.run_batch(first, 100, 0, stream=s))
    jobs.append(j)
    for j in jobs:  # workspaces of these shapes exist before the stall: a growing one would block the host
        j.fill()
        j.late()
        j.enqueue(stream)
    stream.synchronize()
    ended = su.run_jobs(torch, jobs, stream)
    assert not ended, "the stall ended before the calls were enqueued: nothing was held to stream order"
    for j in jobs:
        j.check()


def test_refusals(torch):
    """Each refusal names its code and launches nothing (the outputs keep their sentinel)."""
    from iib_project_ldpc_codes_amd import _native, decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    from tests.graph_util import csr_from_checks
    L = _native.lib()
    g = gu.graph("r36_600")
    bits = torch.zeros((4, g.n), dtype=torch.uint8, device="cuda")
    hard = torch.full((4, g.n), 0x7F, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4 + 21, dtype=torch.int64, device="cuda")

    def decode(graph, b, B=4, iters=20):
        return L.ldpc_gb_decode_batch_dev(None if graph is None else graph.handle(), bits.data_ptr(), B, iters, b, 1,
                                          hard.data_ptr(), None, None)

    def mc(graph, b, B=4, iters=20):
        return L.ldpc_mc_gb_batch_dev(None if graph is None else graph.handle(), 0.03, 1, 0, B, iters, b, 1, -1, 0,
                                      cnt.data_ptr(), None)

    for f in (decode, mc):
        assert f(g, -1) == f(g, 15) == f(None, 0) == f(g, 0, B=-1) == f(g, 0, iters=-1) == _native.LDPC_EINVAL
        assert f(g, 14, B=0) == _native.LDPC_OK
    # one variable of degree 16: check c holds variable 0 and variable c + 1
    wide = TannerGraph.from_csr(*csr_from_checks(np.arange(17) * 2, np.stack([np.zeros(16), np.arange(16) + 1], 1).ravel(), 17))
    assert decode(wide, 0) == mc(wide, 0) == _native.LDPC_EUNSUP
    # past the plan's last fit: n = 40,002 fits at no plane word
    big = gu.graph("r36_40002")
    assert gu.plan("r36_40002", 4, 20, False, False)["name"] == "none"
    assert decode(big, 0) == mc(big, 0) == _native.LDPC_EUNSUP
    torch.cuda.synchronize()
    assert (hard.cpu().numpy() == 0x7F).all() and not cnt.cpu().numpy().any()
    with pytest.raises(ValueError):
        MonteCarlo(g, "awgn", 0.8, 20, algo="gallager")
    with pytest.raises(_native.LdpcError) as e:
        decoder.gallager_decode_dev(g, bits, 20, 15)
    assert e.value.rc == _native.LDPC_EINVAL


def test_montecarlo_run_to_a_frame_error_stop(torch):
    """MonteCarlo.run on r36_600 to 12 frame errors in batches of 100: the reference's sequential counters."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    name, b, p = "r36_600", 0, gu.P_MIX[("r36_600", 0)]
    _, its, curve = gu.decoded(name, p, SEED, 0, BATCH, 20, b, True)
    stop = int((curve[:100, -1] != 0).sum()) + 3  # the stop falls in the second batch
    want = ref.mc_counters(curve, its, -1, stop)
    assert want[1] == stop and 100 < want[0] < 200
    mc = MonteCarlo(gu.graph(name), "bsc", p, 20, algo="gallager", early_stop=True, seed=SEED, batch=100)
    res = mc.run(num_tests=0, stop_frame_errors=stop)
    np.testing.assert_array_equal(res["raw_counters"], want)
    assert res["frame_errors"] == stop and res["num_tests"] == want[0]
