"""Host-only checks of the layered decoder's launch plan (csrc/bp_plan.cpp bp_layer_plan) through
ldpc_debug_layer_plan (no device needed), as literals: which form runs and its grid, LDS and
scratch layout.

One workgroup owns a block P float[n] | R float[E].  It lives wholly in LDS, after the 16-byte
padded Monte-Carlo curve, while curve + block <= 160 KiB - 4 KiB = 159,744 bytes (256 threads, one
workgroup per codeword); past that every workgroup of a grid of one per CU (at most 256) gets a
pad16(4 (n + E))-byte slab of scratch and keeps the block's first (159,744 - curve) / 4 words in
LDS (1024 threads).  A (3,6) graph has 4 n block words: n = 9,984 is the last size whose decode
fits, and its Monte-Carlo calls are pushed off LDS by the curve alone.
"""
import pytest

from tests.graph_util import FALLBACK_KERNELS, bp_plans
from tests.layered_util import LDS_CAP, graph_csr, kernel_name, layer_plans

# algo, early_stop, mc, want_post, iters, B
DECODE, MC = (1, 0, 0, 1, 20, 24), (1, 1, 1, 0, 20, 128)
L8, L16, L32, G8, G16, G32 = 16, 17, 18, 19, 20, 21  # BpPath values, after the flooding and ensemble ones


def _row(p):
    return (p["name"], p["path"], p["threads"], p["grid"], p["lds"], p["lds_slots"], p["slab"], p["scratch"])


def test_plan_rows():
    assert LDS_CAP == 159744
    got = {name: [_row(p) for p in layer_plans(graph_csr(name), [DECODE, MC, (0, 1, 0, 0, 50, 300)])]
           for name in ("r36_600", "r36_9984", "r36_9986", "r36_10000", "r58_8800", "r432_12288", "mixB")}
    assert got["r36_600"] == [("bp_layer_kernel<8,lds>", L8, 256, 24, 9600, 0, 0, 0),
                              ("bp_layer_kernel<8,lds>", L8, 256, 128, 9600 + 96, 0, 0, 0),
                              ("bp_layer_kernel<8,lds>", L8, 256, 300, 9600, 0, 0, 0)]
    # the last (3,6) size in LDS: 4 * 39,936 = 159,744 bytes; the 96-byte curve pushes it off
    assert got["r36_9984"] == [("bp_layer_kernel<8,lds>", L8, 256, 24, 159744, 0, 0, 0),
                               ("bp_layer_kernel<8,gmem>", G8, 1024, 128, 159744, 39912, 128 * 159744, 128 * 159744),
                               ("bp_layer_kernel<8,lds>", L8, 256, 300, 159744, 0, 0, 0)]
    assert got["r36_9986"] == [("bp_layer_kernel<8,gmem>", G8, 1024, 24, 159744, 39936, 24 * 159776, 24 * 159776),
                               ("bp_layer_kernel<8,gmem>", G8, 1024, 128, 159744, 39912, 128 * 159776, 128 * 159776),
                               ("bp_layer_kernel<8,gmem>", G8, 1024, 256, 159744, 39936, 256 * 159776, 256 * 159776)]
    # the headline code: 64 of its 40,000 words in the slab
    assert got["r36_10000"] == [("bp_layer_kernel<8,gmem>", G8, 1024, 24, 159744, 39936, 24 * 160000, 24 * 160000),
                                ("bp_layer_kernel<8,gmem>", G8, 1024, 128, 159744, 39912, 128 * 160000, 128 * 160000),
                                ("bp_layer_kernel<8,gmem>", G8, 1024, 256, 159744, 39936, 256 * 160000, 256 * 160000)]
    assert got["r58_8800"][0] == ("bp_layer_kernel<8,gmem>", G8, 1024, 24, 159744, 39936, 24 * 211200, 24 * 211200)
    assert got["r432_12288"][1] == ("bp_layer_kernel<32,gmem>", G32, 1024, 128, 159744, 39912, 128 * 245760, 128 * 245760)
    assert got["mixB"] == [("bp_layer_kernel<32,lds>", L32, 256, 24, 4 * (700 + 1931), 0, 0, 0),
                           ("bp_layer_kernel<32,lds>", L32, 256, 128, 4 * (700 + 1931) + 96, 0, 0, 0),
                           ("bp_layer_kernel<32,lds>", L32, 256, 300, 4 * (700 + 1931), 0, 0, 0)]


@pytest.mark.parametrize("name", ["r36_600", "r36_10000"] + list(FALLBACK_KERNELS))
def test_plan_invariants(name):
    """Every call shape of tests/test_gpu_layered.py on every graph it runs (and the rest of
    FALLBACK_KERNELS): the form by the block's size, the width by the largest check degree."""
    csr = graph_csr(name)
    n, E = csr[2].size - 1, csr[1].size
    calls = [(algo, es, 0, post, it, B) for algo in (0, 1) for es in (0, 1) for post in (0, 1) for it in (0, 1, 3, 20)
             for B in (8, 24, 264)]
    calls += [(algo, es, 1, 0, 20, 128) for algo in (0, 1) for es in (0, 1)]
    for cus in (256, 8):
        for call, p in zip(calls, layer_plans(csr, calls, cus)):
            mc, iters, B = call[2], call[4], call[5]
            curve = (4 * (iters + 1) + 15) // 16 * 16 if mc else 0
            lds = curve + 4 * (n + E) <= LDS_CAP
            assert p["name"] == kernel_name(csr, lds), (call, p)
            assert p["persistent"] == 0 and p["counter"] == -1, (call, p)
            if lds:
                assert (p["threads"], p["grid"], p["lds"], p["scratch"]) == (256, B, curve + 4 * (n + E), 0), (call, p)
            else:
                assert p["threads"] == 1024 and p["grid"] == min(B, cus), (call, p)
                assert 0 < p["lds_slots"] < n + E, (call, p)
                assert p["lds"] == curve + 4 * p["lds_slots"] == LDS_CAP, (call, p)
                assert p["slab"] == p["scratch"] == p["grid"] * ((4 * (n + E) + 15) // 16 * 16), (call, p)


def test_no_kernel_when_the_curve_alone_fills_lds():
    plans = layer_plans(graph_csr("r36_600"), [(1, 1, 1, 0, 40000, 128), (1, 1, 0, 1, 40000, 128)])
    assert plans[0]["name"] == "none" and plans[0]["scratch"] == 0
    assert plans[1]["name"] == "bp_layer_kernel<8,lds>"  # a decode keeps no curve


def test_flooding_plans_do_not_know_the_schedule():
    """bp_plan's rows of the same calls are what they were: the flooding kernels."""
    for name in ("r36_600", "r58_8800", "mixB"):
        for p in bp_plans(graph_csr(name), [DECODE, MC]):
            assert "layer" not in p["name"] and p["path"] < 10, (name, p)
