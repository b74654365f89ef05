"""The fused codeword / rate-matched Monte-Carlo of the fixed-point decoders
(ldpc_mc_layered_q_cw_batch_dev, MonteCarlo(fused=True)) against the numpy reference of
tests/fused_cw_ref.py.  Every BSC comparison is exact, the whole curve included.

Cases A-D: tests/fused_cw_ref.py.  Seed 7, trials 0 .. 63, 20 iterations.  Figures of the reference,
worked out on the CPU before the assertions were written, as [trials, frame errors, bit errors,
iterations, curve[0]]:

    A  BSC p = 0.05            [64, 7, 82, 330, 254] with early stop, iterations 1,280 without; curve
                               254, 315, 224, 160, ... 84, 82 in both modes (curve[1] > curve[0]: a
                               punctured variable starts as a tie, and a tie decides 0)
    B  BSC p = 0.03            [64, 5, 63, 274, 170]
       BSC p = 0.05            [64, 20, 238, 581, 266]
    C  BSC p = 0.05            [64, 12, 1197, 768, 4920]  (p = 0.03 and 0.04 leave no frame error)
    D  BSC p = 0.06, fixed     [64, 1, 69, 1280, 7133]

Cases E-H (tests/fused_cw_ref.py says what each size is for) hold the codeword mode at 16 and 32 wide,
on bp_qc_q_kernel at 64 and 256 threads and, under qc_util.table_kernels(), on bp_layer_q_kernel<16>
and <32>; fr.FIGURES has their figures, with early stop (iterations 1,280 without, the rest the same):

    E  BSC p = 0.02            [64, 32, 531, 835, 495]    n = 444: the one-dword codeword load, and the
                                                          byte loads on a pointer with & 3 == 1
    F  BSC p = 0.01            [64, 41, 962, 981, 750]    n = 1,220: two-word records, the masked count's
                                                          second round at 64 threads; also with no codeword
    G  BSC p = 0.015           [64, 32, 286, 791, 618]    n = 804, block column 9 shortened, block rows of
                                                          degree 12, 9, 5; curve[1..4] = 725, 641, 433, 378
       count mask mod3         [64, 31, 194, 791, 416]    curve[1..4] = 488, 448, 299, 264
       count="info"            [64, 32, 215, 791, 419]
    H  BSC p = 0.008           [64, 15, 786, 763, 2379]   n = 5,140, block column 16 shortened: the second
                                                          round at 256 threads, two checks per thread
G and H also run without early stop (the barrier after the count is then all that separates it from
the next row's writes), on bp_qc_q_kernel and on the table kernels <16> and <32>; G under mod3 with
max_iters = 0; E-H with no description and no codeword against the all-zero entry and the reference
(the plain Monte-Carlo instantiations of the four wide shapes).

BI-AWGN (r36_1000 with rate_match_ref.classes, sigma = 0.80, B = 192, QUANT): the host chain runs on
ldpc_channel_dev's own values; the bounds are tests/test_gpu_layered_q.py::test_mc_awgn_vs_reference's.
"""
import ctypes as ct

import numpy as np
import pytest

from tests import codeword_util as cu, fused_cw_ref as fr, layered_q_ref, qc_util, rate_match_ref as rr
from tests.test_gpu_fullsize import _dump

pytestmark = pytest.mark.gpu

FIRST = 2 ** 32 - 2  # five trials from here straddle 2^32
FIGURES = {("A", 0.05, True): [64, 7, 82, 330, 254], ("A", 0.05, False): [64, 7, 82, 1280, 254],
           ("B", 0.03, True): [64, 5, 63, 274, 170], ("B", 0.05, True): [64, 20, 238, 581, 266],
           ("B", 0.05, False): [64, 20, 238, 1280, 266], ("C", 0.05, True): [64, 12, 1197, 768, 4920],
           ("D", 0.06, False): [64, 1, 69, 1280, 7133]}
FIGURES.update({k[:3]: v for k, v in fr.FIGURES.items() if k[3] is None})  # E-H under the default mask
KERNEL = {"A": "bp_layer_q_kernel<8>", "B": "bp_qc_q_kernel<64,8>", "C": "bp_qc_q_kernel<256,8>",
          "D": "bp_qc_q_kernel<256,8>", "E": "bp_qc_q_kernel<64,16>", "F": "bp_qc_q_kernel<64,32>",
          "G": "bp_qc_q_kernel<256,16>", "H": "bp_qc_q_kernel<256,32>"}
TABLE = {"B": "bp_layer_q_kernel<8>", "E": "bp_layer_q_kernel<16>", "F": "bp_layer_q_kernel<32>",
         "G": "bp_layer_q_kernel<16>", "H": "bp_layer_q_kernel<32>"}  # the same codes under qc_util.table_kernels()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


_graphs = {}


def _graph(name, table=False):
    """The device graph of a case; table: a quasi-cyclic code on the table kernels (its handle is made
    under LDPC_NO_QC_KERNEL=1)."""
    key = (fr.QC_NAME.get(name, name), table)
    if key not in _graphs:
        if name == "A":
            from iib_project_ldpc_codes_amd.graph import TannerGraph
            _graphs[key] = TannerGraph.random_regular(96, 3, 6, seed=1)
        elif table:
            with qc_util.table_kernels():
                g = qc_util.code(fr.QC_NAME[name]).graph()
                g.handle()
            _graphs[key] = g
        else:
            _graphs[key] = qc_util.graph(fr.QC_NAME[name])
    return _graphs[key]


def _rm(name, count=None):
    """The case's description; count: a mask of fr.MASKS ("info" is RateMatch's own, resolved against the
    graph's encoder; "mod3" goes in as the 0/1 mask itself)."""
    from iib_project_ldpc_codes_amd.ratematch import RateMatch
    if name == "A":
        cls = rr.classes("r36_96")
        return RateMatch(cls.size, cls == rr.PUNCT, cls == rr.KNOWN, "codeword")
    if name == "D":
        return None
    count = "codeword" if count is None else count if count == "info" else np.array(fr.mask(name, count))
    return qc_util.code(fr.QC_NAME[name]).rate_match(punctured_cols=[0], shortened_cols=fr.SHORT_COLS.get(name, []),
                                                     count=count)


def _routed(name, early_stop, table=False, iters=cu.ITERS):
    """The case's plan in the codeword mode, held to the kernel it claims."""
    has_desc = name != "D"
    call = [(1, int(early_stop), 1, 0, iters, fr.B)]
    if name == "A":
        p = fr.layer_q_cw_plans(cu.csr("r36_96"), call, has_desc)[0]
    elif table:
        with qc_util.table_kernels():
            p = fr.qc_cw_plans(qc_util.code(fr.QC_NAME[name]), call, has_desc)[0]
    else:
        p = fr.qc_cw_plans(qc_util.code(fr.QC_NAME[name]), call, has_desc)[0]
    assert p["name"] == (TABLE[name] if table else KERNEL[name]), p
    assert p["grid"] == fr.B
    return p


def _mc(name, p, early_stop, fused=True, table=False, quant=None, count=None, codewords="random", **kw):
    from iib_project_ldpc_codes_amd.decoder import Quant
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    return MonteCarlo(_graph(name, table), "bsc", p, cu.ITERS, algo="minsum", schedule="layered",
                      quant=Quant(*(quant or fr.case(name)["quant"])), early_stop=early_stop, seed=cu.SEED, batch=fr.B,
                      codewords=codewords, rate_match=_rm(name, count), fused=fused, **kw)


def _run(torch, mc, first=0, B=fr.B, stop=0):
    mc.run_batch(first, B, stop)
    torch.cuda.synchronize()
    return mc.counters.cpu().numpy()


# ------------------------------------------------------------------ 1. A-H, bit-exact
@pytest.mark.parametrize("name,p,early_stop,table", [
    ("A", 0.05, True, False), ("A", 0.05, False, False), ("B", 0.03, True, False), ("B", 0.05, True, False),
    ("B", 0.05, False, False), ("B", 0.05, True, True), ("C", 0.05, True, False), ("D", 0.06, False, False),
    ("E", 0.02, True, False), ("F", 0.01, True, False), ("G", 0.015, True, False), ("H", 0.008, True, False),
    ("G", 0.015, False, False), ("H", 0.008, False, False), ("G", 0.015, True, True), ("F", 0.01, True, True),
    ("G", 0.015, False, True), ("H", 0.008, False, True)])  # the table kernels <16> and <32> at a fixed count
def test_counters_equal_the_reference(torch, name, p, early_stop, table):
    _routed(name, early_stop, table)
    want = fr.counters(name, p, early_stop)
    ties = fr.rows(name, p, early_stop)[2]
    assert list(want[:5]) == FIGURES[(name, p, early_stop)]
    assert 0 < want[1] < fr.B and ties > 0  # decoded and failed frames; a tie on a 1 the shortcut would miss
    got = _run(torch, _mc(name, p, early_stop, table=table))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("count,table", [("mod3", False), ("info", False), ("mod3", True)])
def test_count_masks_on_case_g(torch, count, table):
    """An explicit count mask through RateMatch(count=): known and punctured positions counted,
    transmitted ones left out (mod3), and the encoder's information positions (info).  A kernel that
    read no mask, or took "not known" for "counted", gives the default mask's figures instead."""
    p = fr.P_OF["G"]
    _routed("G", True, table)
    want, base = fr.counters("G", p, True, count=count), fr.counters("G", p, True)
    assert list(want[:5]) == fr.FIGURES[("G", p, True, count)]
    assert want[2] != base[2] and want[4] != base[4] and 0 < want[1] < fr.B
    mc = _mc("G", p, True, table=table, count=count)
    assert mc.rate_match.count == ("info" if count == "info" else "mask")
    got = _run(torch, mc)
    np.testing.assert_array_equal(mc.rate_match.counts(), fr.mask("G", count))  # "info": bound to the graph's encoder
    np.testing.assert_array_equal(got, want)


def test_a_description_without_a_codeword(torch):
    """codewords="zero" with rate_match= and fused=True: the entry gets no codeword and means the
    all-zero one, on the 32-wide kernel whose masked count goes a second round (case F)."""
    p = fr.P_OF["F"]
    _routed("F", True)
    want = fr.counters("F", p, True, zero=True)
    assert 0 < want[1] < fr.B and want[4] > 0
    got = _run(torch, _mc("F", p, True, codewords="zero"))
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------- 2. expurgation and a stop inside the batch
def test_expurgation_and_stop_inside_the_batch(torch):
    r, its, _ = fr.rows("B", 0.05, True)
    final = np.asarray(r)[:, -1]
    X = int(final[final > 0].min())
    for ex, stop in ((X, 0), (-1, 10), (X, 10)):
        want = layered_q_ref.mc_counters(np.asarray(r), np.asarray(its), ex, stop)
        if stop:
            assert want[1] == stop and want[0] < fr.B  # the cut falls inside the batch
        else:
            assert want[1] < fr.counters("B", 0.05, True)[1]  # the bound removes a frame error
        got = _run(torch, _mc("B", 0.05, True, expurgation=ex), stop=stop)
        np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------ 3. device identities
@pytest.mark.parametrize("name,p", [("A", 0.05), ("B", 0.05), ("C", 0.05), ("G", 0.015), ("H", 0.008)])
def test_ends_equal_the_unfused_chain(torch, name, p):
    _routed(name, True)
    fused = _run(torch, _mc(name, p, True))
    chain = _run(torch, _mc(name, p, True, fused=False))
    np.testing.assert_array_equal(cu.ends(fused), cu.ends(chain))
    assert not chain[5:-1].any() and fused[5:-1].any()  # the interior is the fused mode's
    # five trials across 2^32
    fused = _run(torch, _mc(name, p, True), FIRST, 5)
    chain = _run(torch, _mc(name, p, True, fused=False), FIRST, 5)
    assert fused[0] == 5
    np.testing.assert_array_equal(cu.ends(fused), cu.ends(chain))


def _entry(torch, g, rm, cw, channel, param, q, B=fr.B, iters=cu.ITERS, early_stop=1, known=1024.0, counters=None,
           first=0):
    from iib_project_ldpc_codes_amd import _native
    if counters is None:
        counters = torch.zeros(_native.MC_NCOUNT + max(iters, 0) + 1, dtype=torch.int64, device="cuda")
    rc = _native.lib().ldpc_mc_layered_q_cw_batch_dev(
        None if g is None else g.handle(), None if rm is None else rm.handle(), None if cw is None else cw.data_ptr(),
        channel, param, known, cu.SEED, first, B, iters, q, early_stop, -1, 0,
        None if counters is False else counters.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, None if counters is False else counters.cpu().numpy()


@pytest.mark.parametrize("name", ["A", "C", "E", "F", "G", "H"])
def test_no_description_no_codeword_equals_the_all_zero_entry(torch, name):
    """E-H: the all-zero Monte-Carlo instantiations of the four wide quasi-cyclic shapes and the
    codeword mode's unmasked count at those widths, both also against the reference."""
    from iib_project_ldpc_codes_amd import _native
    g = _graph(name)
    q = _native.Quant(2.0, 5, 7, 8, 1)
    p = fr.P_OF.get(name, 0.05)
    for early_stop in (1, 0):
        if name in fr.P_OF:
            c, call = qc_util.code(fr.QC_NAME[name]), [(1, early_stop, 1, 0, cu.ITERS, fr.B)]
            assert fr.qc_cw_plans(c, call, 0)[0]["name"] == qc_util.qc_plans(c, call)[0]["name"] == KERNEL[name]
        rc, got = _entry(torch, g, None, None, _native.CH_BSC, p, ct.addressof(q), early_stop=early_stop)
        assert rc == 0, _native.last_error()
        want = torch.zeros(_native.MC_NCOUNT + cu.ITERS + 1, dtype=torch.int64, device="cuda")
        rc = _native.lib().ldpc_mc_layered_q_batch_dev(g.handle(), _native.CH_BSC, p, cu.SEED, 0, fr.B, cu.ITERS,
                                                       ct.addressof(q), early_stop, -1, 0, want.data_ptr(), None)
        assert rc == 0, _native.last_error()
        torch.cuda.synchronize()
        # the BSC's |llr| * scale >= 0.5: no negative LLR quantises to 0, curve[0] agrees as well
        np.testing.assert_array_equal(got, want.cpu().numpy())
        assert got[4] > 0 and got[5] > 0
        if name in fr.P_OF:
            np.testing.assert_array_equal(got, fr.plain_counters(name, p, bool(early_stop)))


def test_scalar_codeword_load_at_a_multiple_of_four(torch):
    """n = 444 (case E): the aligned codeword tensor takes the one-dword load; the same bytes at offset 1
    of a buffer of B n + 4 bytes (pointer & 3 == 1, inside an allocation of the test's) take the byte
    loads at n mod 4 = 0.  Both equal the reference."""
    from iib_project_ldpc_codes_amd import _native
    c, p = fr.case("E"), fr.P_OF["E"]
    assert c["n"] % 4 == 0
    _routed("E", True)
    want = fr.counters("E", p, True)
    assert list(want[:5]) == fr.FIGURES[("E", p, True, None)]
    g, rm, q = _graph("E"), _rm("E"), _native.Quant(2.0, 5, 7, 8, 1)
    x = torch.from_numpy(np.array(c["x"])).cuda()
    buf = torch.zeros(fr.B * c["n"] + 4, dtype=torch.uint8, device="cuda")
    shifted = buf[1:1 + fr.B * c["n"]]
    shifted.copy_(x.reshape(-1))
    assert x.data_ptr() & 3 == 0 and shifted.data_ptr() & 3 == 1 and shifted.data_ptr() == buf.data_ptr() + 1
    for cw in (x, shifted):
        rc, got = _entry(torch, g, rm, cw, _native.CH_BSC, p, ct.addressof(q))
        assert rc == 0, _native.last_error()
        np.testing.assert_array_equal(got, want)


def test_max_iters_zero_on_a_qc_kernel(torch):
    """Case G under the mod3 mask with no iteration: the one entry is the count of the quantised channel
    values, and a counted known position enters with the sign of its quantised +-known_llr."""
    from iib_project_ldpc_codes_amd import _native
    c, p = fr.case("G"), fr.P_OF["G"]
    _routed("G", True, iters=0)
    want = fr.counters("G", p, True, iters=0, count="mod3")
    assert want.size == _native.MC_NCOUNT + 1 and want[2] == want[4] > 0 and want[3] == 0
    assert want[4] != fr.counters("G", p, True, iters=0)[4]  # the mask is seen
    q = _native.Quant(2.0, 5, 7, 8, 1)
    x = torch.from_numpy(np.array(c["x"])).cuda()
    rc, got = _entry(torch, _graph("G"), _rm("G", "mod3"), x, _native.CH_BSC, p, ct.addressof(q), iters=0)
    assert rc == 0, _native.last_error()
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------ 4. BI-AWGN
def test_awgn_on_the_device_stream(torch):
    from iib_project_ldpc_codes_amd import decoder as dec
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    from iib_project_ldpc_codes_amd.ratematch import RateMatch
    name, sigma, B = "r36_1000", 0.80, 192
    cls = rr.classes(name)
    g = TannerGraph.random_regular(1000, 3, 6, seed=1)
    p = fr.layer_q_cw_plans(cu.csr(name), [(1, 1, 1, 0, cu.ITERS, B)], True)[0]
    assert p["name"] == "bp_layer_q_kernel<8>"
    llr0 = dec.channel_dev("awgn", sigma, cu.SEED, 0, 1000, B).cpu().numpy()
    x = rr.codewords(name, B)
    rows, its, ties = fr.rows_of(cu.csr(name), cu.layers(name), cls, x, llr0, cu.QUANT, cu.ITERS, True)
    want = layered_q_ref.mc_counters(rows, its, -1, 0)
    fe, be, ti = int(want[1]), int(want[2]), int(want[3])
    mc = MonteCarlo(g, "awgn", sigma, cu.ITERS, algo="minsum", schedule="layered", quant=dec.Quant(*cu.QUANT),
                    early_stop=True, seed=cu.SEED, batch=B, codewords="random",
                    rate_match=RateMatch(1000, cls == rr.PUNCT, cls == rr.KNOWN, "codeword"), fused=True)
    got = _run(torch, mc, 0, B)
    # what curve[0] would be on the sign of the quantised value instead of the float's
    llr = rr.apply_rules(np.where(x == 1, -llr0, llr0).astype(np.float32), cls, x, False)
    tx = (cls == rr.TX)[None, :]
    by_c = int((((layered_q_ref.quantise(llr, cu.QUANT[2], layered_q_ref.q_of(cu.QUANT[0])) < 0) != (x == 1)) & tx).sum())
    _dump("fused_cw_awgn_r36_1000", {"sigma": sigma, "quant": list(cu.QUANT), "counters_gpu": got[:4].tolist(),
                                     "counters_ref": [B, fe, be, ti], "curve0_gpu": int(got[4]),
                                     "curve0_ref": int(want[4]), "curve0_by_quantised_sign": by_c,
                                     "curve_equal": bool((got == want).all())})
    assert 0 < fe < B and ties > 0
    assert got[0] == B
    assert abs(int(got[1]) - fe) <= 2, (got[:4], fe, be, ti)
    assert abs(int(got[2]) - be) <= 0.02 * be + 20, (got[:4], fe, be)
    assert abs(int(got[3]) - ti) <= 0.005 * ti + 2, (got[:4], ti)
    assert got[4] == want[4] and abs(by_c - int(want[4])) > 100  # the float's sign, not c < 0
    assert got[-1] == got[2]


# ------------------------------------------------------------ 5. refusals and boundaries
def test_entry_refusals_and_boundaries(torch):
    from iib_project_ldpc_codes_amd import _native
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from tests.graph_util import csr_from_checks
    from tests.layered_util import graph as big_graph
    from tests.test_layered_q_ref import INVALID
    g, rm = _graph("A"), _rm("A")
    good = _native.Quant(2.0, 5, 7, 8, 1)
    q = ct.addressof(good)
    BSC, EINVAL, EUNSUP = _native.CH_BSC, _native.LDPC_EINVAL, _native.LDPC_EUNSUP
    x = torch.from_numpy(np.array(fr.case("A")["x"])).cuda()
    assert _entry(torch, g, rm, x, BSC, 0.05, q)[0] == 0
    assert _entry(torch, g, rm, x, _native.CH_BEC, 0.4, q)[0] == EINVAL
    for p in INVALID:
        bad = _native.Quant(p[2], p[0], p[1], p[3], p[4])
        assert _entry(torch, g, rm, x, BSC, 0.05, ct.addressof(bad))[0] == EINVAL, p
    assert _entry(torch, g, rm, x, BSC, 0.7, q)[0] == EINVAL
    for known in (0.0, -1.0, float("inf"), float("nan")):
        assert _entry(torch, g, rm, x, BSC, 0.05, q, known=known)[0] == EINVAL
        # no known position: known_llr is not read
        assert _entry(torch, _graph("B"), _rm("B"), None, BSC, 0.05, q, known=known)[0] == 0
    assert _entry(torch, _graph("B"), rm, None, BSC, 0.05, q)[0] == EINVAL  # a description of another n
    assert _entry(torch, None, rm, x, BSC, 0.05, q)[0] == EINVAL
    assert _entry(torch, g, rm, x, BSC, 0.05, None)[0] == EINVAL
    assert _entry(torch, g, rm, x, BSC, 0.05, q, counters=False)[0] == EINVAL
    assert _entry(torch, g, rm, x, BSC, 0.05, q, B=-1)[0] == EINVAL
    assert _entry(torch, g, rm, x, BSC, 0.05, q, iters=-1)[0] == EINVAL
    # check 0 holds variable 0 twice: no layer schedule
    rows = [[0, 0, 1], [1, 2, 3], [2, 3, 0]]
    twice = TannerGraph.from_csr(*csr_from_checks(np.cumsum([0] + [len(r) for r in rows]), np.concatenate(rows), 4))
    assert _entry(torch, twice, None, None, BSC, 0.05, q)[0] == EUNSUP
    # (3,6) n = 52,000 fits LDS without the codeword's plane (3 n + 32 bytes) and not with it
    big = big_graph("r36_52000")
    counters = torch.zeros(_native.MC_NCOUNT + 6, dtype=torch.int64, device="cuda")
    assert _native.lib().ldpc_mc_layered_q_batch_dev(big.handle(), BSC, 0.01, 1, 0, 1, 5, q, 1, -1, 0, counters.data_ptr(),
                                                     None) == 0
    torch.cuda.synchronize()
    assert _entry(torch, big, None, None, BSC, 0.01, q, B=1, iters=5)[0] == EUNSUP
    # B = 0: a no-op
    seven = torch.full((_native.MC_NCOUNT + cu.ITERS + 1,), 7, dtype=torch.int64, device="cuda")
    rc, got = _entry(torch, g, rm, None, BSC, 0.05, q, B=0, counters=seven)
    assert rc == 0 and (got == 7).all()
    # max_iters = 0: the one entry is the final count, of the quantised channel values
    rc, got = _entry(torch, g, rm, x, BSC, 0.05, q, iters=0)
    assert rc == 0
    want = fr.counters("A", 0.05, True, iters=0)
    assert want[2] == want[4] > 0 and want[3] == 0
    np.testing.assert_array_equal(got, want)


def test_monte_carlo_refusals(torch):
    from iib_project_ldpc_codes_amd.decoder import Quant
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    g, rm, q = _graph("A"), _rm("A"), Quant(*cu.QUANT)
    ok = dict(algo="minsum", schedule="layered", quant=q, codewords="random", rate_match=rm, fused=True)
    MonteCarlo(g, "bsc", 0.05, 5, **ok)
    MonteCarlo(g, "awgn", 0.8, 5, **{**ok, "codewords": "zero"})
    MonteCarlo(g, "bsc", 0.05, 5, **{**ok, "rate_match": None})
    for kind, param, change in (("bsc", 0.05, {"quant": None}), ("bsc", 0.05, {"quant": None, "schedule": "flooding"}),
                                ("bsc", 0.05, {"schedule": "flooding"}), ("bec", 0.4, {"codewords": "zero"}),
                                ("bsc", 0.05, {"codewords": "zero", "rate_match": None}),
                                ("bsc", 0.05, {"algo": "gallager", "quant": None, "schedule": "flooding",
                                               "rate_match": None})):
        with pytest.raises(ValueError, match="fused"):
            MonteCarlo(g, kind, param, 5, **{**ok, **change})


# --------------------------------------------------------------------- 6. queued calls
def test_two_queued_batches_equal_two_synchronised_ones(torch):
    """Stream order: the second batch reuses the first one's buffers and adds to its counters, on a side
    stream and with no host synchronisation between them."""
    side = torch.cuda.Stream()
    queued = _mc("A", 0.05, True)
    torch.cuda.synchronize()
    queued.run_batch(0, 32, 0, stream=side)
    queued.run_batch(32, 32, 0, stream=side)
    side.synchronize()
    synced = _mc("A", 0.05, True)
    for first in (0, 32):
        synced.run_batch(first, 32)
        torch.cuda.synchronize()
    np.testing.assert_array_equal(queued.counters.cpu().numpy(), synced.counters.cpu().numpy())
    np.testing.assert_array_equal(queued.counters.cpu().numpy(), fr.counters("A", 0.05, True))
