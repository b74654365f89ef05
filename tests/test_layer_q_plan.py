"""Host-only checks of the fixed-point layered decoder's launch plan (csrc/bp_plan.cpp
bp_layer_q_plan) through ldpc_debug_layer_q_plan (no device needed), as literals.

One workgroup of 256 threads owns, after the 16-byte padded Monte-Carlo curve, a block
P int8[n] padded to 4 bytes | one record per check (4 bytes up to check degree 16, 8 up to 32),
wholly in LDS: lds = curve + pad4(n) + rec m.  Past 160 KiB - 4 KiB = 159,744 bytes there is no
plan (no slab form).  A (3,6) graph takes pad4(n) + 2 n bytes: n = 53,248 is the last that fits.
"""
import pytest

from tests.graph_util import FALLBACK_KERNELS, bp_plans
from tests.layered_util import LDS_CAP, graph_csr, layer_plans
from tests.layered_q_util import LQ8, LQ16, LQ32, kernel_name, layer_q_plans, lds_bytes

# algo, early_stop, mc, want_post, iters, B
DECODE, MC = (1, 0, 0, 1, 20, 24), (1, 1, 1, 0, 20, 128)
NONE = ("none", 9, 0, 0, 0, 0, 0, 0)  # BpPath::None


def _row(p):
    return (p["name"], p["path"], p["threads"], p["grid"], p["lds"], p["wg_per_cu"], p["slab"], p["scratch"])


def test_plan_rows():
    assert LDS_CAP == 159744
    got = {name: [_row(p) for p in layer_q_plans(graph_csr(name), [DECODE, MC, (1, 1, 0, 0, 50, 300)])]
           for name in ("r36_600", "r36_602", "r36_10000", "r510_640", "r324_1024", "mixA", "mixB")}
    assert got["r36_600"] == [("bp_layer_q_kernel<8>", LQ8, 256, 24, 600 + 4 * 300, 8, 0, 0),
                              ("bp_layer_q_kernel<8>", LQ8, 256, 128, 96 + 600 + 4 * 300, 8, 0, 0),
                              ("bp_layer_q_kernel<8>", LQ8, 256, 300, 600 + 4 * 300, 8, 0, 0)]
    # n no multiple of 4: P padded to 604 bytes
    assert got["r36_602"][0] == ("bp_layer_q_kernel<8>", LQ8, 256, 24, 604 + 4 * 301, 8, 0, 0)
    # the headline code: 30,000 bytes, five workgroups per CU (163,840 / 30,000), also beside a curve
    assert got["r36_10000"] == [("bp_layer_q_kernel<8>", LQ8, 256, 24, 30000, 5, 0, 0),
                                ("bp_layer_q_kernel<8>", LQ8, 256, 128, 30096, 5, 0, 0),
                                ("bp_layer_q_kernel<8>", LQ8, 256, 300, 30000, 5, 0, 0)]
    # the record: 4 bytes at check degree 10, 8 at 24 and 32
    assert got["r510_640"][0] == ("bp_layer_q_kernel<16>", LQ16, 256, 24, 640 + 4 * 320, 8, 0, 0)
    assert got["r324_1024"][0] == ("bp_layer_q_kernel<32>", LQ32, 256, 24, 1024 + 8 * 128, 8, 0, 0)
    assert got["mixA"][1] == ("bp_layer_q_kernel<8>", LQ8, 256, 128, 96 + 1400 + 4 * 1003, 8, 0, 0)
    assert got["mixB"][0] == ("bp_layer_q_kernel<32>", LQ32, 256, 24, 700 + 8 * 144, 8, 0, 0)


def test_fit_boundary():
    """(3,6): pad4(n) + 4 (n / 2) = 159,744 at n = 53,248; the next size has no plan, nor has the
    last one beside a curve."""
    fits = [_row(p) for p in layer_q_plans(graph_csr("r36_53248"), [DECODE, MC])]
    assert fits == [("bp_layer_q_kernel<8>", LQ8, 256, 24, 159744, 1, 0, 0), NONE]
    over = [_row(p) for p in layer_q_plans(graph_csr("r36_53250"), [DECODE, MC])]
    assert over == [NONE, NONE]


@pytest.mark.parametrize("name", ["r36_600", "r36_602", "r36_5060", "r36_10000"] + list(FALLBACK_KERNELS))
def test_plan_invariants(name):
    """Every call shape of tests/test_gpu_layered_q.py on every graph it runs (and the rest of
    FALLBACK_KERNELS): the width by the largest check degree, one workgroup per codeword, no
    scratch, and as many workgroups per CU as LDS and the 32 wave slots hold."""
    csr = graph_csr(name)
    calls = [(1, es, 0, post, it, B) for es in (0, 1) for post in (0, 1) for it in (0, 1, 3, 20) for B in (1, 24, 264)]
    calls += [(1, es, 1, 0, 20, 128) for es in (0, 1)]
    for cus in (256, 8):
        for call, p in zip(calls, layer_q_plans(csr, calls, cus)):
            lds = lds_bytes(csr, call[4], call[2])
            assert lds <= LDS_CAP
            assert p["name"] == kernel_name(csr), (call, p)
            assert (p["threads"], p["grid"], p["lds"]) == (256, call[5], lds), (call, p)
            assert p["wg_per_cu"] == min(8, 160 * 1024 // lds), (call, p)
            assert (p["persistent"], p["counter"], p["slab"], p["scratch"]) == (0, -1, 0, 0), (call, p)


def test_no_kernel_when_the_curve_alone_fills_lds():
    plans = layer_q_plans(graph_csr("r36_600"), [(1, 1, 1, 0, 40000, 128), (1, 1, 0, 1, 40000, 128)])
    assert _row(plans[0]) == NONE
    assert plans[1]["name"] == "bp_layer_q_kernel<8>"  # a decode keeps no curve


def test_the_other_plans_do_not_change():
    """bp_plan's and bp_layer_plan's rows of the same calls know nothing of the new paths."""
    for name in ("r36_600", "r510_640", "mixB"):
        for p in bp_plans(graph_csr(name), [DECODE, MC]):
            assert "layer" not in p["name"] and p["path"] < 10, (name, p)
        for p in layer_plans(graph_csr(name), [DECODE, MC]):
            assert p["name"].startswith("bp_layer_kernel<") and 16 <= p["path"] <= 21, (name, p)
