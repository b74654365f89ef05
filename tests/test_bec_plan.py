"""Host-only checks of the BEC decoders' launch plan (csrc/bec_plan.cpp) through
ldpc_debug_bec_plan, no device needed: which kernel and instantiation a call runs, its
workgroup shape, grid and LDS.  The expected rows are literals worked out from the selection
rules; any change of a rule moves a row.

The rules.  LDS caps: 160 KiB - 1 KiB = 162,816 (bec_kernel, bec_peel_kernel), 160 KiB - 4 KiB =
159,744 (a bit-sliced workgroup), 72 KiB = 73,728 (a bit-sliced workgroup of W > 1 plane words
per variable, or of W = 1 chosen for its grid: two must fit a CU).
  * bec_kernel (one codeword per workgroup): T = 1024 for n >= 4096, else 256;
    LDS = pad16(4 iters) + pad16(n) + m.
  * bit-sliced (batch decode only for B >= 64; fixed-code Monte-Carlo always): T = 512 for
    n > 4096, else 256; the first W of 4, 2, 1 whose u32 planes fit 72 KiB with at least 1,024
    workgroups; else W = 1 on u32 planes under 159,744; else u8 planes, T = 1024, under the same
    cap; else bec_kernel.  A workgroup holds (4 | 8) x plane bytes x W codewords (decode | MC).
  * ensemble Monte-Carlo: bec_peel_kernel when m <= 65,536, dc <= 255, dc n < 2^24 and lists of
    256 entries fit; F = min(m, free bytes / 4), then the test cap; else bec_kernel.
"""
import pytest

from tests.graph_util import BEC_DECODE, BEC_ENS_MC, BEC_MC, bec_plans

WORD_CAP, BITS_CAP, WIDE_CAP = 162816, 159744, 73728
D, M, E = BEC_DECODE, BEC_MC, BEC_ENS_MC

# (mode, n, B, iters) -> (name, kernel, threads, W, plane bytes, codewords per workgroup, LDS, cap); m = n / 2
ROWS = [
    ((D, 96, 63, 5), ("bec_kernel<256>", "Word", 256, 0, 0, 1, 176, WORD_CAP)),
    ((D, 96, 64, 5), ("bec_dec_bits_kernel<256,1,u32>", "DecBits", 256, 1, 4, 16, 660, BITS_CAP)),
    ((D, 96, 32736, 5), ("bec_dec_bits_kernel<256,1,u32>", "DecBits", 256, 1, 4, 16, 660, WIDE_CAP)),
    ((D, 96, 32737, 5), ("bec_dec_bits_kernel<256,2,u32>", "DecBits", 256, 2, 4, 32, 1304, WIDE_CAP)),
    ((D, 96, 65472, 5), ("bec_dec_bits_kernel<256,2,u32>", "DecBits", 256, 2, 4, 32, 1304, WIDE_CAP)),
    ((D, 96, 65473, 5), ("bec_dec_bits_kernel<256,4,u32>", "DecBits", 256, 4, 4, 64, 2592, WIDE_CAP)),
    ((D, 4096, 70, 5), ("bec_dec_bits_kernel<256,1,u32>", "DecBits", 256, 1, 4, 16, 24660, BITS_CAP)),
    ((D, 4098, 70, 5), ("bec_dec_bits_kernel<512,1,u32>", "DecBits", 512, 1, 4, 16, 24676, BITS_CAP)),
    ((D, 10000, 65536, 50), ("bec_dec_bits_kernel<512,1,u32>", "DecBits", 512, 1, 4, 16, 60084, WIDE_CAP)),
    ((D, 26600, 66, 5), ("bec_dec_bits_kernel<512,1,u32>", "DecBits", 512, 1, 4, 16, 159684, BITS_CAP)),
    ((D, 26700, 66, 5), ("bec_dec_bits_kernel<1024,1,u8>", "DecBits", 1024, 1, 1, 4, 40100, BITS_CAP)),
    ((D, 64800, 72, 200), ("bec_dec_bits_kernel<1024,1,u8>", "DecBits", 1024, 1, 1, 4, 97236, BITS_CAP)),
    ((D, 106000, 66, 50), ("bec_dec_bits_kernel<1024,1,u8>", "DecBits", 1024, 1, 1, 4, 159044, BITS_CAP)),
    ((D, 107000, 66, 50), ("bec_kernel<1024>", "Word", 1024, 0, 0, 1, 160716, WORD_CAP)),
    ((D, 109000, 66, 50), ("none", "None", 0, 0, 0, 0, 0, 0)),
    ((M, 96, 3, 5), ("bec_mc_bits_kernel<256,1,u32>", "McBits", 256, 1, 4, 32, 848, BITS_CAP)),
    ((M, 96, 65472, 5), ("bec_mc_bits_kernel<256,1,u32>", "McBits", 256, 1, 4, 32, 848, WIDE_CAP)),
    ((M, 96, 65473, 5), ("bec_mc_bits_kernel<256,2,u32>", "McBits", 256, 2, 4, 64, 1680, WIDE_CAP)),
    ((M, 96, 131072, 5), ("bec_mc_bits_kernel<256,4,u32>", "McBits", 256, 4, 4, 128, 3344, WIDE_CAP)),
    ((M, 1000, 65536, 50), ("bec_mc_bits_kernel<256,2,u32>", "McBits", 256, 2, 4, 64, 12528, WIDE_CAP)),
    ((M, 4098, 70, 5), ("bec_mc_bits_kernel<512,1,u32>", "McBits", 512, 1, 4, 32, 24864, BITS_CAP)),
    ((M, 26600, 66, 5), ("bec_mc_bits_kernel<1024,1,u8>", "McBits", 1024, 1, 1, 8, 39984, BITS_CAP)),
    ((M, 107000, 66, 50), ("bec_kernel<1024>", "Word", 1024, 0, 0, 1, 160716, WORD_CAP)),
]

# ensemble Monte-Carlo: (n, iters, peel_cap) -> (name, kernel, F, LDS, cap)
ENS_ROWS = [
    ((96, 50, 0), ("bec_peel_kernel<1024>", "Peel", 48, 404, WORD_CAP)),
    ((1000, 50, 0), ("bec_peel_kernel<1024>", "Peel", 500, 4192, WORD_CAP)),
    ((10000, 50, 0), ("bec_peel_kernel<1024>", "Peel", 5000, 41880, WORD_CAP)),
    ((64800, 200, 0), ("bec_peel_kernel<1024>", "Peel", 5266, 162816, WORD_CAP)),
    ((64800, 200, 8), ("bec_peel_kernel<1024>", "Peel", 8, 141784, WORD_CAP)),
    ((80000, 50, 0), ("bec_kernel<1024>", "Word", 0, 120208, WORD_CAP)),
    ((110000, 50, 0), ("none", "None", 0, 0, 0)),
]


@pytest.mark.parametrize("call,want", ROWS, ids=[f"{'DM'[c[0]]}-n{c[1]}-B{c[2]}" for c, _ in ROWS])
def test_decode_and_mc_rows(call, want):
    mode, n, B, iters = call
    p, = bec_plans(n, n // 2, [(mode, B, iters)])
    got = (p["name"], p["kernel"], p["threads"], p["W"], p["plane"], p["cw_per_wg"], p["lds"], p["cap"])
    assert got == want
    assert p["F"] == 0
    if p["kernel"] == "Word":
        assert p["grid"] == B
    elif p["kernel"] == "None":
        assert p["grid"] == 0
    else:
        assert p["grid"] == -(-B // p["cw_per_wg"])
        assert p["cw_per_wg"] == (4 if mode == D else 8) * p["plane"] * p["W"]


@pytest.mark.parametrize("call,want", ENS_ROWS, ids=[f"n{c[0]}-cap{c[2]}" for c, _ in ENS_ROWS])
def test_ensemble_rows(call, want):
    n, iters, peel_cap = call
    for B in (1, 40, 4096):
        p, = bec_plans(n, n // 2, [(E, B, iters, peel_cap)])
        assert (p["name"], p["kernel"], p["F"], p["lds"], p["cap"]) == want
        assert p["grid"] == (0 if p["kernel"] == "None" else B) and p["W"] == p["plane"] == 0
        assert p["threads"] == (0 if p["kernel"] == "None" else 1024)
        assert p["cw_per_wg"] == (0 if p["kernel"] == "None" else 1)


def test_peel_limits_other_than_lds():
    """The check word count << 24 | id sum needs dc <= 255 and dc n < 2^24; past either the
    ensemble call runs bec_kernel.  (The third limit, a u16 check id per list entry, m <= 65,536,
    lies beyond the LDS cap: 4 m bytes of check state.)"""
    def name(n, m, dc):
        return bec_plans(n, m, [(E, 8, 20)], dc=dc)[0]["name"]
    assert name(2550, 30, 255) == "bec_peel_kernel<1024>" and name(2560, 30, 256) == "bec_kernel<256>"
    # 255 x 65,793 = 2^24 - 1, 255 x 65,794 = 2^24 + 254
    assert name(65793, 774, 255) == "bec_peel_kernel<1024>" and name(65794, 774, 255) == "bec_kernel<1024>"


def test_width_4_on_512_threads_needs_a_flat_graph():
    """<512,4,u32>: n > 4096 with (n + m) x 16 bytes under 72 KiB -- no rate-1/2 graph, but a
    (3,27) n = 4,104 one (m = 456): 4,560 x 16 + 4 x 64 + 16 + 16 = 73,248 <= 73,728."""
    p, = bec_plans(4104, 456, [(D, 65473, 5)], dc=27)
    assert (p["name"], p["lds"], p["grid"], p["cap"]) == ("bec_dec_bits_kernel<512,4,u32>", 73248, 1024, WIDE_CAP)
    p, = bec_plans(4104, 456, [(D, 65472, 5)], dc=27)  # 1,023 workgroups of 64: two words
    assert p["name"] == "bec_dec_bits_kernel<512,2,u32>"
    p, = bec_plans(4098, 2049, [(D, 65473, 5)])  # rate 1/2: 98,352 bytes of planes at W = 4
    assert p["name"] == "bec_dec_bits_kernel<512,2,u32>"


INSTANTIATIONS = {(256, 1, 4), (256, 2, 4), (256, 4, 4), (512, 1, 4), (512, 2, 4), (512, 4, 4), (1024, 1, 1)}


def test_sweep_none_exactly_where_both_forms_exceed_their_caps():
    """Over n (rate 1/2 and the flat (3,27) shape), B and iters, every mode: no kernel exactly
    where bec_kernel's LDS exceeds 162,816 and the bit-sliced u8 planes (where the mode and
    batch allow them) exceed 159,744; every bit-sliced plan is an instantiation bec.hip has;
    LDS never exceeds the cap it was admitted under."""
    def pad16(x):
        return (x + 15) & ~15
    seen = set()
    shapes = [(n, n // 2, 6) for n in list(range(64, 9000, 331)) + list(range(20000, 120001, 500))]
    shapes += [(n, n // 9, 27) for n in range(4077, 150000, 2997)] + [(4104, 456, 27), (4104, 228, 54)]
    for n, m, dc in shapes:
        calls = [(mode, B, iters) for mode in (D, M, E) for B in (1, 63, 64, 66, 40000, 70000, 140000)
                 for iters in (5, 50, 1000)]
        for (mode, B, iters), p in zip(calls, bec_plans(n, m, calls, dc=dc)):
            word_fits = pad16(4 * iters) + pad16(n) + m <= WORD_CAP
            cw = 4 if mode == D else 8
            bits_fit = (mode == M or (mode == D and B >= 64)) and pad16(n + m) + cw * cw + (4 if mode == D else 0) + 16 <= BITS_CAP
            peel_fits = mode == E and 4 * (m + (n + 31) // 32 + (m + 31) // 32) + 1024 <= WORD_CAP
            assert (p["kernel"] == "None") == (not word_fits and not bits_fit and not peel_fits), (n, m, mode, B, iters, p)
            assert p["lds"] <= p["cap"] <= WORD_CAP
            if p["kernel"] in ("DecBits", "McBits"):
                assert bits_fit and (p["threads"], p["W"], p["plane"]) in INSTANTIATIONS
                assert p["grid"] * p["cw_per_wg"] >= B > (p["grid"] - 1) * p["cw_per_wg"]
                assert p["W"] == 1 or (p["grid"] >= 1024 and p["cap"] == WIDE_CAP)
            if p["kernel"] == "Peel":
                assert peel_fits and (p["F"] == m or p["F"] >= 256)
            seen.add(p["name"])
    assert len(seen) == 2 + 7 + 7 + 1 + 1, sorted(seen)  # every instantiation but none other, and "none"
