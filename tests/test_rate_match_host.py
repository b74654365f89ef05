"""Rate matching without a device: the packed description (ldpc_debug_rate_match_pack) against the numpy
restatement of tests/rate_match_ref.py, its refusals, ratematch.RateMatch and QCCode.rate_match, the
punctured BEC density evolution of de.py, and the snapshot field.  Every comparison is exact unless
stated."""
import numpy as np
import pytest

from iib_project_ldpc_codes_amd import _native, de, qc, ratematch, snapshot
from tests import rate_match_ref as rr


def _random_description(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)


@pytest.mark.parametrize("n", [1, 5, 13, 1000])
@pytest.mark.parametrize("custom", [False, True], ids=["default-count", "custom-count"])
def test_pack_equals_numpy(n, custom):
    cls, cnt = _random_description(n, 100 + n)
    packed, info = ratematch.pack(cls, cnt if custom else None)
    want, want_info = rr.pack(cls, cnt if custom else None)
    assert packed.size == 4 * ((n + 3) // 4)
    np.testing.assert_array_equal(packed, want)
    assert (packed[n:] == rr.PUNCT).all()  # the padding: punctured, uncounted
    assert list(info) == want_info and info[1] + info[2] + info[3] == n
    if not custom:  # the default mask: 1 exactly where the class is not KNOWN
        np.testing.assert_array_equal(packed[:n] >> 2, (cls != rr.KNOWN).astype(np.uint8))


def test_pack_outputs_are_optional():
    cls = np.array([0, 1, 2, 0, 0], np.uint8)
    info = np.zeros(5, np.int32)
    L = _native.lib()
    assert L.ldpc_debug_rate_match_pack(5, cls.ctypes.data, None, None, info.ctypes.data) == 0
    assert list(info) == [5, 3, 1, 1, 4]
    assert L.ldpc_debug_rate_match_pack(5, cls.ctypes.data, None, None, None) == 0


@pytest.mark.parametrize("n,cls,cnt,word", [(1, [3], None, "class"), (4, [0, 1, 2, 255], None, "class"),
                                            (1, [0], [2], "count"), (0, [], None, "n must be"),
                                            (-1, [], None, "n must be")],
                         ids=["class-3", "class-255", "count-2", "n-0", "n-negative"])
def test_pack_refuses(n, cls, cnt, word):
    c = np.array(cls + [0], np.uint8)  # never an empty buffer behind the pointer
    k = None if cnt is None else np.array(cnt, np.uint8)
    rc = _native.lib().ldpc_debug_rate_match_pack(n, c.ctypes.data, None if k is None else k.ctypes.data, None, None)
    assert rc == _native.LDPC_EINVAL and word in _native.last_error()
    assert _native.lib().ldpc_debug_rate_match_pack(1, None, None, None, None) == _native.LDPC_EINVAL


def test_null_handles_are_refused():
    L = _native.lib()
    assert L.ldpc_rate_match_info(None, None, None, None, None, None) == _native.LDPC_EINVAL
    assert L.ldpc_channel_rm_dev(None, 1, 0.1, 1024.0, 0, 0, 0, None, None, None) == _native.LDPC_EINVAL
    assert L.ldpc_mc_rm_count_dev(None, None, None, 1, None, None, 0, 1, -1, 0, None, None) == _native.LDPC_EINVAL
    L.ldpc_rate_match_destroy(None)  # a no-op


# --------------------------------------------------------------- RateMatch, QCCode.rate_match
def test_rate_match_classes_counts_and_rate():
    rm = ratematch.RateMatch(13, punctured=[7, 2], shortened=np.arange(13) == 5)
    assert list(rm.cls) == [0, 0, 1, 0, 0, 2, 0, 1, 0, 0, 0, 0, 0]
    assert (rm.n_tx, rm.n_punct, rm.n_known) == (10, 2, 1)
    np.testing.assert_array_equal(rm.counts(), rr.default_count(rm.cls))
    assert rm.rate(6) == (6 - 1) / 10 == de.rate_matched_rate(6, 10, 1)
    mask = np.zeros(13, np.uint8)
    mask[[0, 5]] = 1
    custom = ratematch.RateMatch(13, [7, 2], [5], count=mask)
    np.testing.assert_array_equal(custom.packed(), rr.pack(rm.cls, mask)[0])
    assert custom.digest() != rm.digest()


def test_count_info_resolves_against_an_encoder():
    class Enc:  # what ratematch reads of an Encoder
        n, info_positions = 13, np.array([0, 1, 2, 3, 4, 5], np.int32)
    rm = ratematch.RateMatch(13, [2, 7], [5], count="info")
    with pytest.raises(ValueError, match="Encoder"):
        rm.counts()
    want = np.zeros(13, np.uint8)
    want[[0, 1, 2, 3, 4]] = 1  # the information positions that are not known; punctured 2 is counted
    np.testing.assert_array_equal(rm.counts(Enc), want)
    np.testing.assert_array_equal(rm.bind(Enc).counts(), want)
    np.testing.assert_array_equal(ratematch.shortened_info_index(Enc, rm), [5])
    u = np.ones((3, 6), np.uint8)
    assert ratematch.shorten_info(u, Enc, rm) is u and (u[:, 5] == 0).all() and (u[:, :5] == 1).all()
    with pytest.raises(ValueError, match="shortened position 9 "):  # the first offender
        ratematch.shortened_info_index(Enc, ratematch.RateMatch(13, [], [11, 9, 4]))


@pytest.mark.parametrize("kw,word", [(dict(punctured=[3, 3]), "given twice"), (dict(shortened=[1, 4, 1]), "given twice"),
                                     (dict(punctured=[3], shortened=[3]), "both punctured and shortened"),
                                     (dict(punctured=[13]), "outside"), (dict(shortened=[-1]), "outside"),
                                     (dict(punctured=np.zeros(12, bool)), "length"), (dict(count="bits"), "count"),
                                     (dict(count=np.full(13, 2)), "count mask")])
def test_rate_match_refuses(kw, word):
    with pytest.raises(ValueError, match=word):
        ratematch.RateMatch(13, **kw)


def test_digest_differs_when_one_class_changes():
    a = ratematch.RateMatch(1000, punctured=[10, 20], shortened=[30])
    b = ratematch.RateMatch(1000, punctured=[10, 21], shortened=[30])
    same = ratematch.RateMatch(1000, punctured=[20, 10], shortened=np.arange(1000) == 30)
    assert a.digest() != b.digest() and a.digest() == same.digest() and len(a.digest()) == 40


def test_qc_block_columns_expand_to_their_variables():
    code = qc.random_base(3, 6, 17, 5)
    rm = code.rate_match(punctured_cols=[0, 1], shortened_cols=[4])
    want = np.zeros(6 * 17, np.uint8)
    want[:34] = rr.PUNCT
    want[4 * 17:5 * 17] = rr.KNOWN
    np.testing.assert_array_equal(rm.cls, want)
    assert (rm.n, rm.n_tx, rm.n_punct, rm.n_known) == (102, 51, 34, 17)
    assert rm.rate(51) == (51 - 17) / 51
    for kw in (dict(punctured_cols=[6]), dict(punctured_cols=[1, 1]), dict(punctured_cols=[2], shortened_cols=[2])):
        with pytest.raises(ValueError):
            code.rate_match(**kw)


# ------------------------------------------------------------------------------ de
def test_punctured_bec_threshold():
    """A fraction pi punctured uniformly at random: the decoder sees the BEC of eps + pi - eps pi, so
    the threshold in eps is 1 - (1 - eps*) / (1 - pi).  Both bisections end within tol = 1e-9 of their
    thresholds: 2e-9 in eps, the unpunctured one scaled by 1 / (1 - pi)."""
    ens = de.regular(3, 6)
    star = de.bec_threshold(ens)
    assert de.bec_threshold(ens, punctured=0.0) == star  # the identical float
    got = de.bec_threshold(ens, punctured=0.1)
    assert abs(got - (1.0 - (1.0 - star) / (1.0 - 0.1))) <= 2e-9 / 0.9
    with pytest.raises(ValueError):
        de.bec_threshold(ens, punctured=1.0)


def test_punctured_bec_de():
    ens = de.regular(3, 6)
    assert de.bec_de(ens, 0.4, 30, punctured=0.0) == de.bec_de(ens, 0.4, 30)
    assert de.bec_de(ens, 0.3, 30, punctured=0.125) == de.bec_de(ens, 0.3 + 0.125 - 0.3 * 0.125, 30)


def test_rate_matched_rate():
    assert de.rate_matched_rate(500, 900, 40) == 460 / 900
    for bad in ((500, 0, 0), (500, 900, 501), (500, 900, -1)):
        with pytest.raises(ValueError):
            de.rate_matched_rate(*bad)


# ----------------------------------------------------------------------- MonteCarlo, snapshots
def _mc(rm=None, **kw):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo

    def executor(first_cw, B, stop, counters):
        counters[0] += B
    g = TannerGraph.random_regular(96, 3, 6, seed=1)
    return MonteCarlo(g, kw.pop("channel", "bsc"), 0.05, 10, algo=kw.pop("algo", "minsum"), batch=8, executor=executor,
                      rate_match=rm, **kw)


def test_snapshot_field_only_with_a_description():
    plain = _mc().snapshot()
    assert "rate_match" not in plain["config"]
    rm = ratematch.RateMatch(96, [1, 2], [3])
    snap = _mc(rm, known_llr=512.0).snapshot()
    assert snap["config"]["rate_match"] == {"sha1": rm.digest(), "known_llr": 512.0}
    rest = {k: v for k, v in snap["config"].items() if k != "rate_match"}
    assert rest == plain["config"]  # nothing else moves


def test_restore_across_two_descriptions_raises():
    a, b = ratematch.RateMatch(96, [1, 2], [3]), ratematch.RateMatch(96, [1, 2], [4])
    mc = _mc(a)
    mc.run(num_tests=16, stop_frame_errors=0)
    snap = mc.snapshot()
    again = _mc(a)
    again.restore(snap)
    assert again.next_trial() == 16
    for other in (_mc(b), _mc(None), _mc(a, known_llr=64.0)):
        with pytest.raises(ValueError, match="different run configuration"):
            other.restore(snap)
    with pytest.raises(ValueError, match="different run configuration"):
        _mc(a).restore(_mc().snapshot())


def test_montecarlo_refusals_need_no_device():
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    rm = ratematch.RateMatch(96, [1, 2], [3])
    with pytest.raises(ValueError, match="n = 95"):
        _mc(ratematch.RateMatch(95, [1]))
    with pytest.raises(ValueError, match="punctured"):
        _mc(rm, algo="gallager")
    _mc(ratematch.RateMatch(96, [], [3]), algo="gallager")  # known positions alone are fine
    with pytest.raises(ValueError, match="fixed code"):
        MonteCarlo.ensemble(96, 3, 6, "bsc", 0.05, 10, rate_match=rm, executor=lambda *a: None)
    with pytest.raises(ValueError, match="ML"):
        _mc(rm, channel="bec", algo="spa", optimal=True)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="known_llr"):
            _mc(rm, known_llr=bad)


# ------------------------------------------------------------------------------ fer_sweep.py
def _fer_sweep():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fer_sweep", os.path.join(root, "scripts", "fer_sweep.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fer_sweep_flags(tmp_path):
    fs = _fer_sweep()
    assert fs.parse_indices("3,7,10-12") == [3, 7, 10, 11, 12]
    path = tmp_path / "fill.txt"
    path.write_text("40-42\n50, 51\n")
    assert fs.parse_indices("@" + str(path)) == [40, 41, 42, 50, 51]
    args = fs.parse(["qc", "--array", "3,6,17", "--puncture-cols", "0,1", "--shorten", "@" + str(path)])
    g = qc.array_code(3, 6, 17).graph()
    rm = fs.rate_match_of(args, g)
    np.testing.assert_array_equal(rm.punctured, np.arange(34))
    np.testing.assert_array_equal(rm.shortened, [40, 41, 42, 50, 51])
    assert rm.rate(g.n - g.m) == (51 - 5) / (102 - 34 - 5)  # what the sweep's rate and Eb/N0 are computed from
    assert fs.rate_match_of(fs.parse(["qc", "--array", "3,6,17"]), g) is None
    for bad in (["cfg3", "--puncture-cols", "0"], ["ens", "--puncture", "1"], ["cfg3", "--shorten", "x"]):
        with pytest.raises(SystemExit):
            fs.parse(bad)
