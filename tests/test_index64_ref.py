"""The reference side of the 64-bit trial-index tests (CPU only): the oracle is what
tests/test_gpu_index64.py takes it for at seeds, trial indices and graph indices with non-zero high
words, and the host driver carries such indices exactly.

* The BEC / BSC channel equals the rule of DESIGN 3.4 computed from the Philox block that
  tests/test_oracle_golden.py pins with the Random123 known-answer vectors.
* Trial t (graph t) is the same whatever batch it is drawn in, across 2^32.
* Every case of tests/index64_util.py tells the three bug models of wrong_index_models from the
  truth, by the oracle alone: what the device test compares would differ under each of them.
* MonteCarlo on an oracle-backed executor, restored just below 2^32: exact Python-int first_cw on
  both sides of 2^32 on one rank and on two gloo ranks, counters equal to the oracle's, the trial
  range exact through JSON, and a frame-error stop behind the crossing cutting at the right trial.
"""
import json
import os

import numpy as np
import pytest
import torch

from iib_project_ldpc_codes_amd import snapshot
from oracle import oracle
from tests import index64_util as u
from tests.index64_util import M, SEED, T, wrong_index_models  # noqa: F401  (wrong_index_models: exported)
from tests.test_multiprocess import _spawn


# ------------------------------------------------------------------ the channel rule
@pytest.mark.parametrize("seed,cw", [(SEED, T + 5), (0x1234_5678_9ABC_DEF1, 0xFFFF_FFFF_0000_0001 - 2),
                                     (0x0000_0001_0000_0001, 0x7FFF_FFFF_FFFF_FFFE), (SEED, 5 * T - 1)])
@pytest.mark.parametrize("n", [7, 1003])
def test_channel_is_the_philox_rule_at_high_words(seed, cw, n):
    assert all(x != 0 for x in (seed & M, seed >> 32, cw & M, cw >> 32))
    p = 0.3
    u01 = np.zeros(n, np.float64)
    for v in range(n):
        x = int(oracle.philox([v >> 2, 0, cw & M, cw >> 32], [seed & M, seed >> 32])[v & 3])
        u01[v] = (2 * (x >> 9) + 1) * 2.0 ** -24
    hit = u01 < float(np.float32(p))
    assert n < 100 or 0.2 * n < hit.sum() < 0.4 * n  # both outcomes occur, about p of them hits
    np.testing.assert_array_equal(oracle.channel(oracle.CH_BEC, p, seed, cw, n, 1)[0], np.where(hit, 2, 0))
    p2 = np.float32(oracle.channel_params(oracle.CH_BSC, p)[1])
    np.testing.assert_array_equal(oracle.channel(oracle.CH_BSC, p, seed, cw, n, 1)[0], np.where(hit, -p2, p2))


# --------------------------------------------------------------- batch independence
@pytest.mark.parametrize("kind", ["bec", "bsc", "awgn"])
def test_channel_batch_straddling_equals_its_halves(kind):
    k, p = u.CH_KIND[kind], {"bec": 0.4, "bsc": 0.07, "awgn": 0.8}[kind]
    whole = oracle.channel(k, p, SEED, T - 3, 1003, 8)
    np.testing.assert_array_equal(whole[:3], oracle.channel(k, p, SEED, T - 3, 1003, 3))
    np.testing.assert_array_equal(whole[3:], oracle.channel(k, p, SEED, T, 1003, 5))


@pytest.mark.parametrize("n,dv,dc", [(1000, 3, 6), (2732, 3, 6)])
def test_regular_sampler_batch_straddling_equals_its_halves(n, dv, dc):
    """One-level sampler below 8,192 edges, sequential-draw sampler from there on."""
    assert (n * dv >= u.SEQ_E) == (n == 2732)
    whole = oracle.sample_regular_batch(n, dv, dc, SEED, T - 3, 8)
    lo = oracle.sample_regular_batch(n, dv, dc, SEED, T - 3, 3)
    hi = oracle.sample_regular_batch(n, dv, dc, SEED, T, 5)
    for w, a, b in zip(whole, lo, hi):
        np.testing.assert_array_equal(w, np.concatenate([a, b]))
    one = oracle.sample_regular(n, dv, dc, SEED, T + 1)
    for w, a in zip(whole, one):
        np.testing.assert_array_equal(w[4], a)


def test_csr_sampler_is_keyed_by_the_whole_graph_index():
    vptr, cptr = u.csr_ptrs(2000)
    a = oracle.sample_csr(vptr, cptr, SEED, T + 1)
    b = oracle.sample_csr(vptr, cptr, SEED, T + 1)
    low = oracle.sample_csr(vptr, cptr, SEED, 1)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[2] == b[2] > 0 and not np.array_equal(a[0], low[0])


# ------------------------------------------------------------ discriminating inputs
def test_wrong_index_models():
    m = wrong_index_models(T - 3, 8, SEED)
    assert m["index_high_dropped"][0] == [T - 3, T - 2, T - 1, 0, 1, 2, 3, 4]
    assert m["index_high_without_carry"][0] == m["index_high_dropped"][0]
    assert m["seed_high_dropped"] == ([T - 3 + b for b in range(8)], SEED & M) and SEED >> 63 == 1
    m = wrong_index_models(3 * T - 1, 3, 7)
    assert m["index_high_dropped"][0] == [T - 1, 0, 1]
    assert m["index_high_without_carry"][0] == [3 * T - 1, 2 * T, 2 * T + 1]


@pytest.mark.parametrize("name", sorted(u.BY_NAME))
def test_case_tells_every_wrong_index_model_from_the_truth(name):
    c = u.BY_NAME[name]
    first, B = c["first"], c["B"]
    assert first < T < first + B  # the batch straddles: trial 2^32 is neither its first nor beyond it
    truth = u.want(c)
    for model, (idx, seed) in wrong_index_models(first, B, SEED).items():
        wrong = u.expected(c, idx, seed)
        assert any(not np.array_equal(a, b) for a, b in zip(truth, wrong)), (name, model)
        if c["family"] in ("channel", "bec_ens", "sampler") and model != "seed_high_dropped":
            # per-trial results: the trials below 2^32 agree, the first one at or above it differs
            off = T - first
            assert all(np.array_equal(a[:off], b[:off]) for a, b in zip(truth, wrong))
            assert any(not np.array_equal(a[off], b[off]) for a, b in zip(truth, wrong))


@pytest.mark.parametrize("name", [c["name"] for c in u.SOFT_CASES + u.SOFT_ENS_CASES + u.LAYER_CASES
                                  + u.LAYER_Q_CASES + [u.DRIVER_CASE]])
def test_soft_case_has_decoded_and_failed_frames(name):
    c = u.BY_NAME[name]
    for w in u.want(c):
        assert w[0] == c["B"] and 0 < w[1] < c["B"], (name, w[:4])


def test_bec_stop_case_cuts_behind_the_crossing():
    c = u.BY_NAME["bec-bits-96-65473-X1-stop"]
    w = u.want(c)[0]
    plain = u.want(u.BY_NAME["bec-bits-96-65473"])[0]
    assert 0 < w[1] < plain[1] and w[0] < c["B"]
    assert c["first"] + int(w[0]) - 1 >= T + 8  # the last counted trial


def test_sequential_sampler_case_sits_on_the_threshold():
    c = u.BY_NAME["sample-seq-2732"]
    assert c["n"] * c["dv"] == 8196 >= u.SEQ_E > (c["n"] - 2) * c["dv"]


# -------------------------------------------------------------------- host plumbing
N, ITERS, B, EPS = 200, 20, 32, 0.42
BASE = T - B - B // 2  # where the restored run continues


def _graph():
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    return TannerGraph.random_regular(N, 3, 6, seed=5)


def _oracle_counters(g, first, count, remaining=0):
    words = oracle.channel(oracle.CH_BEC, EPS, SEED, first, g.n, count)
    _, err, its = oracle.bec_decode_batch(words, ITERS, g.variable_lookup, g.check_lookup, g.n, g.k, g.dv, g.dc)
    curve = np.concatenate([np.count_nonzero(words == 2, axis=1)[:, None], err], axis=1)
    return u.counters(curve, its, -1, remaining)


def _mc(g, calls):
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo

    def executor(first_cw, Bn, stop, counters):
        calls.append((first_cw, Bn, type(first_cw).__name__))
        rem = int(stop - counters[1]) if stop else 0
        if stop and rem <= 0:
            return
        counters += torch.from_numpy(_oracle_counters(g, first_cw, Bn, rem))
    return MonteCarlo(g, "bec", EPS, ITERS, seed=SEED, batch=B, executor=executor)


def _snapshot_below_the_crossing(g, path):
    """A snapshot of trials [BASE - B, BASE) as a run of one batch would have written it."""
    mc = _mc(g, [])
    snap = mc.snapshot()
    snap["trial_ranges"] = [[BASE - B, BASE]]
    snap["counters"] = [int(x) for x in _oracle_counters(g, BASE - B, B)]
    snapshot.save(snap, path)
    return snapshot.load(path)


def test_restored_run_crosses_2_32_on_one_rank(tmp_path):
    g = _graph()
    path = str(tmp_path / "run.json")
    snap = _snapshot_below_the_crossing(g, path)
    assert snap["seed"] == SEED and snap["trial_ranges"] == [[T - 80, T - 48]]
    calls = []
    mc = _mc(g, calls)
    mc.restore(snap)
    res = mc.run(num_tests=4 * B, stop_frame_errors=0, checkpoint=path)
    assert calls == [(T - 48, B, "int"), (T - 16, B, "int"), (T + 16, B, "int")]
    np.testing.assert_array_equal(res["raw_counters"], _oracle_counters(g, BASE - B, 4 * B))
    saved = json.loads(open(path).read())
    assert saved["trial_ranges"] == [[T - 80, T + 48]] and saved["seed"] == SEED
    assert all(type(x) is int for x in saved["trial_ranges"][0] + [saved["seed"]])
    again = _mc(g, [])
    again.restore(snapshot.load(path))
    assert again.next_trial() == T + 48


def test_frame_error_stop_behind_the_crossing_cuts_at_the_right_trial(tmp_path):
    g = _graph()
    snap = _snapshot_below_the_crossing(g, str(tmp_path / "run.json"))
    upto = _oracle_counters(g, BASE - B, (T + 5) - (BASE - B) + 1)  # the trials up to 2^32 + 5
    stop = int(upto[1]) + 2
    want = _oracle_counters(g, BASE - B, 8 * B, remaining=stop)
    assert want[1] == stop and BASE - B + int(want[0]) - 1 > T + 5  # the cut trial, from the oracle alone
    mc = _mc(g, [])
    mc.restore(snap)
    res = mc.run(num_tests=0, stop_frame_errors=stop)
    np.testing.assert_array_equal(res["raw_counters"], want)
    assert mc.snapshot()["trial_ranges"] == [[BASE - B, BASE - B + int(want[0])]]


def _resume_worker(rank, world, port, path, num_tests, stop, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        calls = []
        mc = _mc(_graph(), calls)
        mc.restore(snapshot.load(path))
        res = mc.run(num_tests=num_tests, stop_frame_errors=stop)
        q.put((rank, calls, res["raw_counters"].tolist(), mc.snapshot()["trial_ranges"]))
    finally:
        dist.destroy_process_group()


def test_restored_run_crosses_2_32_on_two_ranks(tmp_path):
    """Three rounds of two ranks: rank r of round R runs [BASE + (2 R + r) B, + B)."""
    g = _graph()
    path = str(tmp_path / "run.json")
    _snapshot_below_the_crossing(g, path)
    out = _spawn(_resume_worker, 2, path, 7 * B, 0)
    want = _oracle_counters(g, BASE - B, 7 * B)
    for rank, calls, c, ranges in out:
        assert calls == [(BASE + (2 * R + rank) * B, B, "int") for R in range(3)]
        np.testing.assert_array_equal(np.array(c), want)
        assert ranges == [[T - 80, T - 80 + 7 * B]]
    firsts = sorted(f for _, calls, _, _ in out for f, _, _ in calls)
    assert firsts[0] < T - B and firsts[1] < T < firsts[1] + B and firsts[2] > T


def test_frame_error_stop_behind_the_crossing_on_two_ranks(tmp_path):
    g = _graph()
    path = str(tmp_path / "run.json")
    _snapshot_below_the_crossing(g, path)
    upto = _oracle_counters(g, BASE - B, (T + 5) - (BASE - B) + 1)
    stop = int(upto[1]) + 2
    want = _oracle_counters(g, BASE - B, 8 * B, remaining=stop)
    assert want[1] == stop
    for rank, calls, c, ranges in _spawn(_resume_worker, 2, path, 0, stop):
        np.testing.assert_array_equal(np.array(c), want)
        assert ranges == [[BASE - B, BASE - B + int(want[0])]]
