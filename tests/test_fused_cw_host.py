"""The fused codeword Monte-Carlo without a device: the reference's own ends against the unfused host
chain, the launch plans of the codeword mode (ldpc_debug_layer_q_cw_plan, ldpc_debug_qc_cw_plan; host
only), MonteCarlo(fused=True) on a stand-in executor (results, snapshot, refusals) and
scripts/fer_sweep.py --fused's argument validation."""
import importlib.util
import os

import numpy as np
import pytest

from tests import codeword_util as cu, fused_cw_ref as fr, gallager_ref, qc_util, rate_match_ref as rr
from tests.layered_util import LDS_CAP, graph_csr
from tests.layered_q_util import LQ8, layer_q_plans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# algo, early_stop, mc, want_post, iters, B
MC, MC50, DECODE = (1, 1, 1, 0, 20, 128), (1, 1, 1, 0, 50, 65536), (1, 0, 0, 1, 20, 24)
NONE = ("none", 9, 0, 0, 0, 0)  # BpPath::None


def _row(p):
    return (p["name"], p["path"], p["threads"], p["grid"], p["lds"], p["wg_per_cu"])


# ------------------------------------------------------------------------- the reference
def test_reference_ends_equal_the_unfused_host_chain():
    want = fr.counters("A", 0.05, True)
    assert list(want[:5]) == [64, 7, 82, 330, 254]
    rows, its, _ = rr.chain("r36_96", 0.05, 64, "layered_q")
    chain = gallager_ref.mc_counters(rows, its, -1, 0)
    np.testing.assert_array_equal(cu.ends(want), cu.ends(chain))
    assert not chain[5:-1].any()
    assert list(want[4:]) == [254, 315, 224, 160, 123, 105, 95, 85, 83, 83, 77, 67, 76, 69, 79, 69, 70, 71, 76, 84, 82]
    fixed = fr.counters("A", 0.05, False)
    assert list(fixed[:5]) == [64, 7, 82, 1280, 254] and list(fixed[4:]) == list(want[4:])


# ----------------------------------------------------------------------------- the plans
def test_plan_rows_of_the_table_kernel():
    assert fr.plane_bytes(600) == 76 and fr.plane_bytes(10000) == 1252 and fr.plane_bytes(96) == 12
    for name, n in (("r36_600", 600), ("r36_602", 602), ("r36_10000", 10000)):
        csr = graph_csr(name)
        old = layer_q_plans(csr, [MC, MC50])
        for has_desc in (0, 1):
            new = fr.layer_q_cw_plans(csr, [MC, MC50], has_desc)
            for o, p in zip(old, new):
                lds = o["lds"] + fr.plane_bytes(n)  # a description adds nothing: its count mask is re-read
                assert _row(p) == (o["name"], LQ8, 256, o["grid"], lds, min(8, 160 * 1024 // lds)), (name, has_desc, p)
                assert (p["persistent"], p["counter"], p["slab"], p["scratch"]) == (0, -1, 0, 0)
    # the headline shape: 208 + 10,000 + 20,000 + 1,252 bytes, five workgroups per CU, with a description too
    head = [_row(p) for h in (0, 1) for p in fr.layer_q_cw_plans(graph_csr("r36_10000"), [MC50], h)]
    assert head == 2 * [("bp_layer_q_kernel<8>", LQ8, 256, 65536, 31460, 5)]


def test_plan_cap_and_the_mode_is_monte_carlo_only():
    from iib_project_ldpc_codes_amd import _native
    assert LDS_CAP == 159744
    # (3,6) n = 52,000 with a curve of 6: 32 + 156,000 bytes fit; the codeword's plane of 6,500 does not
    csr = graph_csr("r36_52000")
    call = [(1, 1, 1, 0, 5, 1)]
    assert _row(layer_q_plans(csr, call)[0]) == ("bp_layer_q_kernel<8>", LQ8, 256, 1, 156032, 1)
    assert fr.layer_q_cw_plans(csr, call, 0, rc_only=True) == _native.LDPC_EUNSUP
    assert fr.layer_q_cw_plans(csr, call, 1, rc_only=True) == _native.LDPC_EUNSUP
    # n = 51,000: 153,032 + 6,376 = 159,408 fit, with a description too
    csr = graph_csr("r36_51000")
    for has_desc in (0, 1):
        assert _row(fr.layer_q_cw_plans(csr, call, has_desc)[0]) == ("bp_layer_q_kernel<8>", LQ8, 256, 1, 159408, 1)
    # a decode has no codeword mode
    assert fr.layer_q_cw_plans(graph_csr("r36_600"), [DECODE], 0, rc_only=True) == _native.LDPC_EUNSUP
    assert fr.layer_q_cw_plans(graph_csr("r36_600"), [MC], 0, rc_only=True) == 0


def test_plan_rows_of_the_qc_kernels():
    for name in ("rnd36_z17", "rnd36_z307", "hand_z31", "dense2x20_z23"):
        c = qc_util.code(name)
        old = qc_util.qc_plans(c, [MC])[0]
        assert old["name"] == qc_util.kernel_name(c)
        for has_desc in (0, 1):
            p = fr.qc_cw_plans(c, [MC], has_desc)[0]
            lds = old["lds"] + fr.plane_bytes(c.n)
            T = 64 if c.Z <= 64 else 256
            assert _row(p) == (old["name"], old["path"], T, 128, lds, min(32 // (T // 64), 160 * 1024 // lds)), (name, p)
    with qc_util.table_kernels():  # the block-row schedule on the table kernels
        p = fr.qc_cw_plans(qc_util.code("rnd36_z17"), [MC], 1)[0]
    assert p["name"] == "bp_layer_q_kernel<8>" and p["lds"] == 96 + 104 + 4 * 51 + 16


WIDE = {"E": ("bp_qc_q_kernel<64,16>", 64, 16), "F": ("bp_qc_q_kernel<64,32>", 64, 32),
        "G": ("bp_qc_q_kernel<256,16>", 256, 16), "H": ("bp_qc_q_kernel<256,32>", 256, 32)}


@pytest.mark.parametrize("name", sorted(WIDE))
def test_plan_rows_of_the_wide_cases(name):
    """Cases E-H of tests/fused_cw_ref.py: the 16- and 32-wide codeword-mode kernels by name, and the
    block curve | P | records of one or two words | plane."""
    kernel, T, wide = WIDE[name]
    c = qc_util.code(fr.QC_NAME[name])
    assert (c.n % 4, c.n % 32 != 0) == (0, True)  # the one-dword codeword load; a partial plane word
    lds = fr.curve_bytes(cu.ITERS) + 4 * ((c.n + 3) // 4) + (4 if wide == 16 else 8) * c.m + fr.plane_bytes(c.n)
    for early_stop in (0, 1):
        call = [(1, early_stop, 1, 0, cu.ITERS, fr.B)]
        for has_desc in (0, 1):
            p = fr.qc_cw_plans(c, call, has_desc)[0]
            assert (p["name"], p["threads"], p["grid"], p["lds"]) == (kernel, T, fr.B, lds), (name, p)
            with qc_util.table_kernels():
                p = fr.qc_cw_plans(c, call, has_desc)[0]
            assert (p["name"], p["threads"], p["grid"], p["lds"]) == ("bp_layer_q_kernel<%d>" % wide, 256, fr.B, lds)
    # what the sizes are for: the masked count's second round at F and H, with a ragged tail
    n4 = c.n // 4
    assert (n4 > 4 * T and n4 % T != 0) == (name in "FH")


@pytest.mark.parametrize("key", sorted(fr.FIGURES, key=str))
def test_reference_figures_of_the_wide_cases(key):
    name, p, early_stop, count = key
    want = fr.counters(name, p, early_stop, count=count)
    assert list(want[:5]) == fr.FIGURES[key]
    assert 0 < want[1] < fr.B and fr.rows(name, p, early_stop, count=count)[2] > 0  # ties on a 1
    if (name, count) in fr.CURVE_1_4:
        assert list(want[5:9]) == fr.CURVE_1_4[(name, count)]
    assert want[-1] == want[2]
    cls, Z = fr.case(name)["cls"], qc_util.code(fr.QC_NAME[name]).Z
    short = [c for c in range(cls.size // Z) if (cls[c * Z:(c + 1) * Z] == rr.KNOWN).all()]
    assert (cls[:Z] == rr.PUNCT).all() and short == fr.SHORT_COLS.get(name, [])  # block column 0 punctured


def test_reference_masks_differ_from_the_default():
    """A kernel that ignored the count mask would give the default mask's figures: both explicit masks
    of case G move the bit errors and curve[0], and mod3 hides one frame error."""
    cls, p = fr.case("G")["cls"], fr.P_OF["G"]
    base = fr.counters("G", p, True)
    assert int(fr.mask("G", None).sum()) == 804 - 67
    for count in ("mod3", "info"):
        m = fr.mask("G", count)
        assert int(m.sum()) == 536
        got = fr.counters("G", p, True, count=count)
        assert got[2] != base[2] and got[4] != base[4] and got[3] == base[3]
    m = fr.mask("G", "mod3")
    assert (m[cls == rr.KNOWN] == 1).any() and (m[cls == rr.PUNCT] == 1).any() and (m[cls == rr.TX] == 0).any()
    assert not fr.mask("G", "info")[cls == rr.KNOWN].any()
    assert fr.counters("G", p, True, count="mod3")[1] == base[1] - 1  # a frame whose errors all lie uncounted
    # max_iters = 0 under mod3: the counted known positions enter, with the sign of +known_llr quantised (no error)
    zero = fr.counters("G", p, True, iters=0, count="mod3")
    assert zero[2] == zero[4] > 0 and zero[3] == 0 and zero[4] != fr.counters("G", p, True, iters=0)[4]
    # the all-zero word under a description (case F): decoded and failed frames
    z = fr.counters("F", fr.P_OF["F"], True, zero=True)
    assert 0 < z[1] < fr.B and list(z[:5]) != fr.FIGURES[("F", 0.01, True, None)]


# ---------------------------------------------------------- MonteCarlo(fused=True) on a stand-in
B, ITERS = 32, 10


def _executor(first_cw, batch, stop_frame_errors, counters, stream=None):
    counters[0] += batch
    counters[1] += 1
    counters[4:] += 3  # every curve entry counted


def _mc(fused, **kw):
    from iib_project_ldpc_codes_amd.decoder import Quant
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    g = TannerGraph.random_regular(120, 3, 6, seed=1)
    args = dict(algo="minsum", seed=5, batch=B, executor=_executor, schedule="layered", quant=Quant(5, 7, 2.0, 8, 1),
                codewords="random")
    args.update(kw)
    return MonteCarlo(g, "bsc", 0.07, ITERS, fused=fused, **args) if fused is not None else \
        MonteCarlo(g, "bsc", 0.07, ITERS, **args)


def test_results_keep_the_interior_only_when_fused():
    res = _mc(True).run(2 * B, stop_frame_errors=0)
    assert np.isfinite(res["error_curve"]).all() and res["error_curve"][3] == 6 / (120 * 2 * B)
    res = _mc(False).run(2 * B, stop_frame_errors=0)
    assert np.isnan(res["error_curve"][1:-1]).all() and np.isfinite(res["error_curve"][[0, -1]]).all()


def test_snapshot_records_fused_and_refuses_the_other_mode(tmp_path):
    from iib_project_ldpc_codes_amd import snapshot
    a = _mc(True)
    a.run(2 * B, stop_frame_errors=0)
    assert snapshot.config(a)["fused"] is True
    plain = snapshot.config(_mc(False))
    assert "fused" not in plain and plain == snapshot.config(_mc(None))  # the unfused snapshot is what it was
    assert {k: v for k, v in snapshot.config(a).items() if k != "fused"} == plain
    path = str(tmp_path / "f.json")
    snapshot.save(a.snapshot(), path)
    b = _mc(True)
    b.restore(snapshot.load(path))
    assert b.next_trial() == 2 * B
    with pytest.raises(ValueError):
        _mc(False).restore(snapshot.load(path))
    c = _mc(False)
    c.run(B, stop_frame_errors=0)
    with pytest.raises(ValueError):
        _mc(True).restore(c.snapshot())
    with pytest.raises(ValueError):
        snapshot.merge([a.snapshot(), c.snapshot()])


def test_what_fused_needs():
    from iib_project_ldpc_codes_amd.ratematch import RateMatch
    rm = RateMatch(120, [0, 1, 2], [])
    _mc(True, codewords="zero", rate_match=rm)
    _mc(True, rate_match=rm)
    for change in ({"quant": None}, {"quant": None, "schedule": "flooding"}, {"schedule": "flooding"},
                   {"codewords": "zero"}, {"algo": "gallager", "quant": None, "schedule": "flooding"}):
        with pytest.raises(ValueError, match="fused"):
            _mc(True, **change)
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    with pytest.raises(ValueError, match="fused"):
        MonteCarlo(TannerGraph.random_regular(120, 3, 6, seed=1), "bec", 0.4, ITERS, rate_match=rm, fused=True,
                   executor=_executor)


# ------------------------------------------------------------------- scripts/fer_sweep.py --fused
def _sweep():
    spec = importlib.util.spec_from_file_location("fer_sweep", os.path.join(ROOT, "scripts", "fer_sweep.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fer_sweep_fused_arguments(capsys):
    fs = _sweep()
    q = ["--schedule", "layered", "--quant", "5,7,2.0,8,1"]
    assert fs.parse(["cfg3"]).fused is False
    assert fs.parse(["cfg3", *q, "--codewords", "random", "--fused"]).fused is True
    assert fs.parse(["cfg3", *q, "--puncture", "0-9", "--fused"]).fused is True
    assert fs.parse(["qc", "--array", "3,6,17", *q, "--puncture-cols", "0", "--fused"]).fused is True
    for argv in (["cfg3", "--codewords", "random", "--fused"], ["cfg3", "--schedule", "layered", "--codewords", "random", "--fused"],
                 ["cfg3", *q, "--fused"], ["cfg4", "--codewords", "random", "--fused"], ["ens", "--fused"]):
        with pytest.raises(SystemExit):
            fs.parse(argv)
        assert "--fused" in capsys.readouterr().err
