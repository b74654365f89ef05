"""The two restatements of Gallager A/B (tests/gallager_ref.py) held to each other and to cases worked
by hand, the density evolution of iib_project_ldpc_codes_amd/de.py, and the snapshot fields of a
Gallager run.  No device."""
import numpy as np
import pytest

from tests import gallager_ref as ref
from tests.graph_util import csr_from_checks
from tests.layered_util import graph_csr

GRAPHS = ("r36_600", "r48_256", "mixA", "mixB")


def _words(n, B, p, seed):
    return (np.random.default_rng(seed).random((B, n)) < p).astype(np.uint8)


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("b,early_stop", [(0, True), (0, False), (1, True), (2, True), (2, False)])
def test_sequential_and_vectorised_forms_agree(name, b, early_stop):
    csr = graph_csr(name)
    n = csr[2].size - 1
    Y = _words(n, 3, 0.004 if name == "mixB" else 0.03, seed=7)
    Y[2] = _words(n, 1, 0.5, seed=8)  # a dense word: nothing converges
    for iters in (0, 1, 6):
        hard, its, curve = ref.decode(csr, Y, iters, b, early_stop)
        for r in range(Y.shape[0]):
            h1, i1, c1 = ref.decode_word(csr, Y[r], iters, b, early_stop)
            np.testing.assert_array_equal(hard[r], h1)
            assert its[r] == i1
            np.testing.assert_array_equal(curve[r], c1)


# Three variables on two checks: c0 = {v0, v1}, c1 = {v1, v2}; v1 has degree 2, v0 and v2 degree 1
_CHAIN = csr_from_checks(np.array([0, 2, 4]), np.array([0, 1, 1, 2]), 3)


def test_hand_worked_chain():
    """y = 1 0 0.  v0 and v2 (degree 1) always send y.  Iteration 1: c0 tells v1 "1", c1 tells v1 "0";
    v1 has D = 1 of d = 2, 2 D > d + 1 fails: x1 = 0; v0 hears 0 from c0: D = 1, d = 1, 2 > 2 fails:
    x0 = y0 = 1.  x = 1 0 0 violates c0, so nothing stops; the degree-1 variables never change, and v1
    sends c0 the flip of y1 when the other message disagrees (b_d = 1 = d - 1 for A and B): it sends 0 ^
    [dis(c1) >= 1] = 0 to c0 and 0 ^ [dis(c0) >= 1] = 1 to c1.  Iteration 2: c1 now tells v2 "1": v2
    has D = 1, d = 1: x2 = 0 still.  The decisions stay 1 0 0 for ever."""
    for b in (0, 1):
        for es in (False, True):
            hard, its, curve = ref.decode(_CHAIN, np.array([[1, 0, 0]]), 4, b, es)
            np.testing.assert_array_equal(hard, [[1, 0, 0]])
            assert its[0] == 4
            np.testing.assert_array_equal(curve, [[1, 1, 1, 1, 1]])
            assert ref.decode_word(_CHAIN, [1, 0, 0], 4, b, es) == ([1, 0, 0], 4, [1, 1, 1, 1, 1])


# One variable of degree 3 corrected by its three checks: v0 on c0, c1, c2, each check closed by its own
# degree-1 variable (v1, v2, v3)
_STAR = csr_from_checks(np.array([0, 2, 4, 6]), np.array([0, 1, 0, 2, 0, 3]), 4)


def test_hand_worked_star():
    """y = 1 0 0 0: every check tells v0 "0", D = 3 of d = 3, 2 D = 6 > 4: x0 = 0.  v0 tells each leaf
    "1" in iteration 1 (messages start as y), a leaf has D = 1, d = 1 and keeps y = 0: x = 0 after one
    iteration, all checks hold, its = 1."""
    hard, its, curve = ref.decode(_STAR, np.array([[1, 0, 0, 0]]), 5, 0, True)
    np.testing.assert_array_equal(hard, [[0, 0, 0, 0]])
    assert its[0] == 1
    np.testing.assert_array_equal(curve, [[1, 0, 0, 0, 0, 0]])
    assert ref.decode_word(_STAR, [1, 0, 0, 0], 5, 0, True) == ([0, 0, 0, 0], 1, [1, 0, 0, 0, 0, 0])


@pytest.mark.parametrize("name", GRAPHS)
def test_zero_word_stops_after_one_iteration(name):
    csr = graph_csr(name)
    n = csr[2].size - 1
    hard, its, curve = ref.decode(csr, np.zeros((2, n), np.uint8), 5, 0, True)
    assert not hard.any() and (its == 1).all() and not curve.any()


@pytest.mark.parametrize("name", GRAPHS)
def test_no_iterations_returns_the_word(name):
    csr = graph_csr(name)
    Y = _words(csr[2].size - 1, 3, 0.1, seed=3)
    for es in (False, True):
        hard, its, curve = ref.decode(csr, Y | 0xFE, 0, 1, es)  # only bit 0 is read
        np.testing.assert_array_equal(hard, Y)
        assert (its == 0).all()
        np.testing.assert_array_equal(curve[:, 0], Y.sum(axis=1))


@pytest.mark.parametrize("name,dv", [("r36_600", 3), ("r48_256", 4)])
def test_a_is_b_at_dv_minus_1_on_a_regular_graph(name, dv):
    csr = graph_csr(name)
    Y = _words(csr[2].size - 1, 8, 0.03, seed=5)
    a = ref.decode(csr, Y, 8, 0, True)
    for b in (dv - 1, dv, 14):  # min(b, d - 1)
        for x, z in zip(a, ref.decode(csr, Y, 8, b, True)):
            np.testing.assert_array_equal(x, z)


def test_check_holding_a_variable_twice():
    """c0 = {v0, v0, v1}: v0's two slots cancel in the check's XOR towards v1 (v1 hears 0 ^ 0 or 1 ^ 1 =
    0), and each of v0's slots hears the other slot's bit ^ v1's.  y = 0 1: v1 (degree 1) hears 0,
    D = 1, keeps y1 = 1; v0 hears 0 ^ 1 = 1 on both slots, D = 2 of d = 2, 2 D = 4 > 3: x0 = 1.  x = 1 1
    has syndrome 1 ^ 1 ^ 1 = 1: no stop.  v0 then sends y0 ^ [D - dis_j >= 1] = 1 on both slots; v1
    hears 1 ^ 1 = 0 again and v0 hears 1 ^ 1 = 0: D = 0, x0 = 0.  x = 0 1 from then on."""
    csr = csr_from_checks(np.array([0, 3]), np.array([0, 0, 1]), 2)
    for b in (0, 1):
        hard, its, curve = ref.decode(csr, np.array([[0, 1]]), 3, b, True)
        assert ref.decode_word(csr, [0, 1], 3, b, True) == ([int(x) for x in hard[0]], int(its[0]), [int(x) for x in curve[0]])
        assert curve[0, 0] == 1 and curve[0, 1] == 2 and its[0] == 3


# ------------------------------------------------------------------------ density evolution
def test_gallager_a_threshold_of_the_3_6_ensemble():
    from iib_project_ldpc_codes_amd import de
    t = de.gallager_threshold(3, 6, 0)
    assert abs(t - 0.0394636562) < 1e-9
    assert de.gallager_threshold(3, 6, 2) == t  # b = 0 is b = dv - 1


def test_gallager_de_is_monotone_in_p():
    from iib_project_ldpc_codes_amd import de
    assert de.gallager_de(3, 6, 0, 0.03, 30) == de.gallager_de(3, 6, 2, 0.03, 30)
    for dv, dc, b in ((3, 6, 0), (4, 8, 0), (4, 8, 2), (5, 10, 3)):
        prev = de.gallager_de(dv, dc, b, 0.001, 40)
        assert prev[0] == 0.001 and len(prev) == 41
        for p in (0.005, 0.01, 0.02, 0.04, 0.08):
            cur = de.gallager_de(dv, dc, b, p, 40)
            assert all(c >= q for c, q in zip(cur, prev))
            prev = cur
    assert de.gallager_de(3, 6, 0, 0.039, 2000)[-1] < 1e-12 < de.gallager_de(3, 6, 0, 0.040, 2000)[-1]


# --------------------------------------------------------------------------------- snapshot
class _Run:
    """What snapshot.config reads of a MonteCarlo."""

    def __init__(self, **kw):
        from iib_project_ldpc_codes_amd.graph import TannerGraph
        self.graph = TannerGraph.random_regular(24, 3, 6, seed=1)
        self.channel, self.param, self.max_iters, self.algo, self.alpha = 1, 0.03, 20, 1, 0.75
        self.early_stop, self.expurgation, self.optimal, self.message_passing = True, -1, False, True
        self.schedule, self.quant, self.gallager = "flooding", None, False
        self.__dict__.update(kw)


def test_snapshot_config_fields():
    from iib_project_ldpc_codes_amd import snapshot
    ms = snapshot.config(_Run())
    fp = snapshot.graph_fingerprint(_Run().graph)
    # a flooding min-sum run: the keys and values of every snapshot written before this field existed
    assert ms == {"graph": fp, "channel": 1, "param": 0.03, "max_iters": 20, "algo": 1, "alpha": 0.75,
                  "early_stop": True, "expurgation": -1, "optimal": False, "message_passing": True}
    assert list(ms) == ["graph", "channel", "param", "max_iters", "algo", "alpha", "early_stop", "expurgation",
                        "optimal", "message_passing"]
    gb = snapshot.config(_Run(gallager=True, algo="gallager", flip_threshold=2))
    assert gb == {**ms, "algo": "gallager", "flip_threshold": 2}


def test_restore_refuses_another_algorithm():
    import torch
    from iib_project_ldpc_codes_amd import snapshot
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    g = _Run().graph
    run = lambda **kw: MonteCarlo(g, "bsc", 0.03, 5, seed=3, batch=8, executor=lambda *a: None, **kw)  # noqa: E731
    a = run(algo="gallager", flip_threshold=1)
    snap = a.snapshot(np.zeros(len(a.counters), np.int64))
    assert snap["config"]["algo"] == "gallager" and snap["config"]["flip_threshold"] == 1
    run(algo="gallager", flip_threshold=1).restore(snap)
    for other in (run(algo="gallager", flip_threshold=0), run(algo="minsum"), run(algo="spa")):
        with pytest.raises(ValueError):
            other.restore(snap)
    assert isinstance(a.counters, torch.Tensor)


def test_montecarlo_refuses_what_gallager_does_not_decode():
    from iib_project_ldpc_codes_amd.decoder import Quant
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    g = _Run().graph
    ex = lambda *a: None  # noqa: E731
    for kw in (dict(channel="awgn"), dict(channel="bec"), dict(schedule="layered"),
               dict(quant=Quant(6, 8, 2.0)), dict(flip_threshold=15), dict(flip_threshold=-1)):
        ch = kw.pop("channel", "bsc")
        with pytest.raises(ValueError):
            MonteCarlo(g, ch, 0.03 if ch != "awgn" else 0.8, 5, algo="gallager", executor=ex, **kw)
    with pytest.raises(ValueError):
        MonteCarlo.ensemble(24, 3, 6, "bsc", 0.03, 5, algo="gallager", executor=ex)
    with pytest.raises(ValueError):
        MonteCarlo(g, "bsc", 0.03, 5, algo="minsum", flip_threshold=2, executor=ex)
