"""gb_plan (csrc/gb_plan.cpp, read through ldpc_debug_gb_plan without a device): literal rows of the
plane ladder, invariants over every call shape tests/test_gpu_gallager.py uses, and the other plans'
rows on the same calls.

The ladder: the widest plane word of u32, u16, u8 whose planes -- one word per slot and per variable,
a second per variable under early stop or Monte-Carlo -- fit 160 KiB - 4 KiB beside 4 bytes per codeword
of the workgroup and 16 bytes of flags; 256 threads up to n = 2,048, 1,024 beyond.  The rows below were
worked out from that rule by hand: lds = pad16((E + n [+ n]) * plane) + 32 * plane + 16.
"""
import pytest

from tests import gallager_util as gu
from tests.graph_util import BEC_DECODE, BEC_MC, bec_plans, bp_plans

CAP = 160 * 1024 - 4096


def _row(threads, plane, grid, lds, scratch, name):
    return {"threads": threads, "W": 1, "plane": plane, "cw_per_wg": 8 * plane, "grid": grid, "lds": lds, "cap": CAP,
            "scratch": scratch, "name": name}


NONE = {"threads": 0, "W": 0, "plane": 0, "cw_per_wg": 0, "grid": 0, "lds": 0, "cap": 0, "scratch": 0, "name": "none"}
# the four calls of every graph: (B, iters, early_stop, mc)
CALLS = [(264, 20, 0, 0), (264, 20, 1, 0), (264, 20, 1, 1), (33, 50, 0, 1)]
TRIAL = 4 * 264 * 22, 4 * 33 * 52  # trial rows [B][iters + 1] and iteration counts [B], int32

ROWS = {
    # n = 600, E = 1,800: 2,400 words * 4 = 9,600 (+ 144); with X 3,000 * 4 = 12,000
    "r36_600": [_row(256, 4, 9, 9744, 0, "gb_kernel<256,u32>"), _row(256, 4, 9, 12144, 0, "gb_kernel<256,u32,es>"),
                _row(256, 4, 9, 12144, TRIAL[0], "gb_kernel<256,u32,es,mc>"),
                _row(256, 4, 2, 12144, TRIAL[1], "gb_kernel<256,u32,mc>")],
    # n = 602 (no multiple of 4), E = 1,806: 2,408 * 4 = 9,632; with X 3,010 * 4 = 12,040 -> 12,048 padded
    "r36_602": [_row(256, 4, 9, 9776, 0, "gb_kernel<256,u32>"), _row(256, 4, 9, 12192, 0, "gb_kernel<256,u32,es>"),
                _row(256, 4, 9, 12192, TRIAL[0], "gb_kernel<256,u32,es,mc>"),
                _row(256, 4, 2, 12192, TRIAL[1], "gb_kernel<256,u32,mc>")],
    # n = 10,000, E = 30,000: u32 planes are 160,000 (200,000 with X) > 159,744 - 144: the 16-bit word,
    # 80,000 + 80 and 100,000 + 80
    "r36_10000": [_row(1024, 2, 17, 80080, 0, "gb_kernel<1024,u16>"), _row(1024, 2, 17, 100080, 0, "gb_kernel<1024,u16,es>"),
                  _row(1024, 2, 17, 100080, TRIAL[0], "gb_kernel<1024,u16,es,mc>"),
                  _row(1024, 2, 3, 100080, TRIAL[1], "gb_kernel<1024,u16,mc>")],
    # n = 700, E = 1,931: 2,631 * 4 = 10,524 -> 10,528; with X 3,331 * 4 = 13,324 -> 13,328
    "mixB": [_row(256, 4, 9, 10672, 0, "gb_kernel<256,u32>"), _row(256, 4, 9, 13472, 0, "gb_kernel<256,u32,es>"),
             _row(256, 4, 9, 13472, TRIAL[0], "gb_kernel<256,u32,es,mc>"),
             _row(256, 4, 2, 13472, TRIAL[1], "gb_kernel<256,u32,mc>")],
    # n = 32,000, E = 96,000: a plain decode's u8 planes are 128,000; with X 160,000: past the last fit
    "r36_32000": [_row(1024, 1, 33, 128048, 0, "gb_kernel<1024,u8>"), NONE, NONE, NONE],
    # n = 40,002, E = 120,006: 160,008 bytes even without X
    "r36_40002": [NONE, NONE, NONE, NONE],
}


def _shape(name):
    if name.startswith("r36_"):  # the plan reads the shape alone: no graph is drawn
        n = int(name.split("_")[1])
        return n, 3 * n
    return gu.shape(name)[:2]


@pytest.mark.parametrize("name", sorted(ROWS))
def test_literal_rows(name):
    n, E = _shape(name)
    assert gu.gb_plans(n, E, CALLS) == ROWS[name]


def _gpu_test_calls():
    """(graph, B, iters, early_stop, mc) of every call tests/test_gpu_gallager.py makes."""
    from tests import test_gpu_gallager as t
    return t.plan_calls()


def test_invariants_over_the_gpu_tests_calls():
    calls = _gpu_test_calls()
    assert len(calls) > 100
    seen = set()
    for name, B, iters, es, mc in calls:
        n, E = _shape(name)
        p = gu.gb_plans(n, E, [(B, iters, es, mc)])[0]
        assert p["threads"] in (256, 1024) and p["plane"] in (4, 2, 1) and p["W"] == 1, (name, p)
        assert p["cw_per_wg"] == 8 * p["plane"]
        planes = (E + (2 if es or mc else 1) * n) * p["plane"]
        assert p["lds"] == (planes + 15) // 16 * 16 + 4 * p["cw_per_wg"] + 16
        assert p["lds"] <= p["cap"] == CAP
        assert p["grid"] == -(-B // p["cw_per_wg"])
        assert p["scratch"] == (4 * B * (iters + 2) if mc else 0)  # the trial rows and nothing else
        # the next wider plane word would not have fitted
        assert p["plane"] == 4 or 2 * planes + 8 * p["cw_per_wg"] + 16 > CAP
        seen.add(p["name"])
    modes = ("", ",es", ",mc", ",es,mc")
    assert seen == {"gb_kernel<%s%s>" % (s, m) for s in ("256,u32", "1024,u32", "1024,u16", "1024,u8") for m in modes}


# The other plans on the same graphs and calls: the rows of the parent commit, written down from it
BP_ROWS = {
    "r36_600": [("bp_lds_kernel<3,6>", 256, 256, 7600), ("bp_loc_kernel", 256, 264, 5152)],
    "mixB": [("bp_generic_kernel<32,lds>", 256, 264, 12464), ("bp_generic_kernel<32,lds>", 256, 264, 12548)],
}


@pytest.mark.parametrize("name", sorted(BP_ROWS))
def test_soft_plans_unchanged(name):
    # (algo, early_stop, mc, want_post, iters, B): a min-sum decode and a sum-product early-stop Monte-Carlo
    plans = bp_plans(gu.graph_csr(name), [(1, 0, 0, 1, 20, 264), (0, 1, 1, 0, 20, 264)])
    assert [(p["name"], p["threads"], p["grid"], p["lds"]) for p in plans] == BP_ROWS[name]


def test_bec_plans_unchanged():
    rows = bec_plans(600, 300, [(BEC_DECODE, 264, 20), (BEC_MC, 264, 20)]) + bec_plans(10000, 5000, [(BEC_MC, 65536, 50)])
    assert [(p["name"], p["threads"], p["W"], p["plane"], p["grid"], p["lds"]) for p in rows] == [
        ("bec_dec_bits_kernel<256,1,u32>", 256, 1, 4, 17, 3684),
        ("bec_mc_bits_kernel<256,1,u32>", 256, 1, 4, 9, 3872),
        ("bec_mc_bits_kernel<512,1,u32>", 512, 1, 4, 2048, 60272)]
