"""Host-only checks of the graph samplers' launch plan (csrc/sample_plan.cpp) through
ldpc_debug_sample_plan, no device needed: which draw kernel a shape runs, its workgroup and LDS,
the ring, counter and row widths, the variable-side kernel's chunks and the search pass's grid.
The expected rows are literals worked out from the selection rules; any change of a rule moves a row.

The rules, for n variables, m checks, E sockets, the largest check / variable degree:
  * sequential-draw sampler for 8,192 <= E <= 393,216 with check degrees <= 192: 128 threads,
    bw = (E + 31) / 32 rounded up to 4 bitmap words, a ring of 512 u16 entries for n <= 65,536, else
    of int; LDS = 4 (bw + 344) + (2 | 4) 512.  Counters of fb = 2 / 4 / 8 bits up to variable degree
    3 / 15 / 255, fb = 0 from 256.  mdv = ceil(2^32 / dv) for 2 <= dv <= 255 (regular), else 0.
  * variable side (fb > 0): rows of u16 entries when m <= 65,536 (regular: check ids) or
    E <= 65,536 (CSR: slot ids), else int32; V = min(n, 150 KiB * 8 / (8 (2 | 4) max_vdeg + fb))
    rounded down to 64 variables per workgroup, nch = ceil(n / V) workgroups per graph, LDS =
    V fb / 8 + (2 | 4) V max_vdeg.  V = 0 (fewer than 64 variables, or fb = 0): the emit pass builds
    the variable side itself, from the counters when n of them fit the bitmap, else by global CAS.
  * search pass (a device given): per_cu = min(32, 160 KiB / LDS) workgroups per CU, W = min(G,
    cus per_cu).
  * otherwise one Rao-Sandelius level of K = 256 (E <= 16,384) / 512 (E < 65,536) buckets with the
    permutation as u16 in LDS, LDS = 4 (K K / 64 + 16) + 2 E -- or, from E = 65,536 or with a
    variable id past u16 (n > 65,536), 1024 buckets on the global row, LDS = 65,600.
"""
import pytest

from tests import sampler_shapes_util as u
from tests.sampler_shapes_util import ONE256, ONE512, ONE1024, SEQ_CI, SEQ_CU, SEQ_RI, SEQ_RU, VS16, VS32, sample_plan


def R(n, dv, dc, G=6):
    return (n, n * dv // dc, n * dv, dc, dv, True, dv, G)


def C(n, m, E, cdeg, vdeg, G=6):
    return (n, m, E, cdeg, vdeg, False, 0, G)


# (n, m, E, max_cdeg, max_vdeg, regular, dv, G) -> (draw kernel, threads, K, ring bytes, fb, V, nch, row bytes, W at
# 256 CUs)
ROWS = [
    # E = 8,191 | 8,192 and 393,216 | 393,217
    (C(4000, 2730, 8191, 3, 3), (ONE256, 256, 256, 0, 0, 0, 0, 0, 0)),
    (C(4000, 2730, 8192, 3, 3), (SEQ_CU, 128, 0, 2, 2, 3968, 2, 2, 6)),
    (C(60000, 131072, 393216, 3, 7), (SEQ_CU, 128, 0, 2, 4, 5376, 12, 4, 6)),
    (C(60000, 131072, 393217, 3, 7), (ONE1024, 1024, 1024, 0, 0, 0, 0, 0, 0)),
    # the bucket thresholds E = 16,384 | 16,385 and 65,535 | 65,536 (a check of degree 193)
    (C(5000, 5000, 16384, 193, 4), (ONE256, 256, 256, 0, 0, 0, 0, 0, 0)),
    (C(5000, 5000, 16385, 193, 4), (ONE512, 512, 512, 0, 0, 0, 0, 0, 0)),
    (C(20000, 20000, 65535, 193, 4), (ONE512, 512, 512, 0, 0, 0, 0, 0, 0)),
    (C(20000, 20000, 65536, 193, 4), (ONE1024, 1024, 1024, 0, 0, 0, 0, 0, 0)),
    # check degree 192 | 193
    (C(6000, 3748, 12000, 192, 2), (SEQ_CU, 128, 0, 2, 2, 5952, 2, 2, 6)),
    (C(6000, 3748, 12000, 193, 2), (ONE256, 256, 256, 0, 0, 0, 0, 0, 0)),
    # n = 65,536 | 65,537 (here also m: the ring and the rows widen together)
    (R(65536, 2, 2), (SEQ_RU, 128, 0, 2, 2, 36096, 2, 2, 6)),
    (R(65537, 2, 2), (SEQ_RI, 128, 0, 4, 2, 18560, 4, 4, 6)),
    # m = 65,536 | 65,537 under an int ring (regular); dv = 1: no reciprocal
    (R(131072, 1, 2), (SEQ_RI, 128, 0, 4, 2, 68224, 2, 2, 6)),
    (R(131074, 1, 2), (SEQ_RI, 128, 0, 4, 2, 36096, 4, 4, 6)),
    # E = 65,536 | 65,537 (CSR rows hold slot ids)
    (C(30000, 20000, 65536, 4, 3), (SEQ_CU, 128, 0, 2, 2, 24576, 2, 2, 6)),
    (C(30000, 20000, 65537, 4, 3), (SEQ_CU, 128, 0, 2, 2, 12480, 3, 4, 6)),
    # variable degree 3 | 4, 15 | 16, 255 | 256
    (C(6000, 4000, 12000, 3, 3), (SEQ_CU, 128, 0, 2, 2, 5952, 2, 2, 6)),
    (C(6000, 4000, 12000, 3, 4), (SEQ_CU, 128, 0, 2, 4, 5952, 2, 2, 6)),
    (C(6000, 4000, 12000, 3, 15), (SEQ_CU, 128, 0, 2, 4, 4992, 2, 2, 6)),
    (C(6000, 4000, 12000, 3, 16), (SEQ_CU, 128, 0, 2, 8, 4608, 2, 2, 6)),
    (C(6000, 4000, 12000, 3, 255), (SEQ_CU, 128, 0, 2, 8, 256, 24, 2, 6)),
    (C(6000, 4000, 12000, 3, 256), (SEQ_CU, 128, 0, 2, 0, 0, 0, 2, 6)),
    # dv = 1 | 2
    (R(8192, 1, 2), (SEQ_RU, 128, 0, 2, 2, 8192, 1, 2, 6)),
    (R(4096, 2, 4), (SEQ_RU, 128, 0, 2, 2, 4096, 1, 2, 6)),
    # V = n | V < n
    (R(24576, 3, 6), (SEQ_RU, 128, 0, 2, 2, 24576, 1, 2, 6)),
    (R(24640, 3, 6), (SEQ_RU, 128, 0, 2, 2, 24576, 2, 2, 6)),
    # fewer than 64 variables: no variable-side kernel
    (R(60, 255, 3), (SEQ_RU, 128, 0, 2, 8, 0, 0, 2, 6)),
    (C(63, 4000, 12000, 3, 255), (SEQ_CU, 128, 0, 2, 8, 0, 0, 2, 6)),
    # variable ids past u16 below 65,536 sockets (degree-0 variables): 1024 buckets on the global row
    (C(66000, 2000, 6000, 3, 2), (ONE1024, 1024, 1024, 0, 0, 0, 0, 0, 0)),
    (C(65536, 2000, 6000, 3, 2), (ONE256, 256, 256, 0, 0, 0, 0, 0, 0)),
]


@pytest.mark.parametrize("shape,want", ROWS, ids=[f"{'R' if s[5] else 'C'}-n{s[0]}-E{s[2]}-c{s[3]}-v{s[4]}" for s, _ in ROWS])
def test_rows(shape, want):
    p = sample_plan(*shape)
    got = (p["draw"], p["threads"], p["K"], p["ring"], p["fb"], p["V"], p["nch"], p["row"], p["W"])
    assert got == want
    csr = "csr" if not shape[5] else "regular"
    if p["seq"]:
        assert p["search"] == f"sample_search_kernel<{csr},{'u16' if p['ring'] == 2 else 'int'}>"
        assert p["var_side"] == ("none" if not p["V"] else VS16 if p["row"] == 2 else VS32)
    else:
        assert (p["search"], p["var_side"], p["bw"], p["emit_fb"], p["mdv"]) == ("none", "none", 0, 0, 0)


def test_lds_bytes_and_counter_placement():
    """LDS literals of the carves, and where the counters live (fbu, the emit pass's argument)."""
    def f(shape, *keys):
        p = sample_plan(*shape)
        return tuple(p[k] for k in keys)
    assert f(C(4000, 2730, 8191, 3, 3), "lds") == (4 * (256 * 4 + 16) + 2 * 8191,)
    assert f(C(20000, 20000, 65535, 193, 4), "lds") == (4 * (512 * 8 + 16) + 2 * 65535,)  # 147,518
    assert f(C(66000, 2000, 6000, 3, 2), "lds") == (4 * (1024 * 16 + 16),)  # the 1024-bucket carve, whatever E
    assert f(R(4096, 2, 4), "lds", "bw") == (4 * (256 + 344) + 1024, 256)
    assert f(R(2731, 3, 3), "lds", "bw") == (4 * (260 + 344) + 1024, 260)  # 257 words, rounded up to 4
    assert f(R(131072, 3, 6), "lds", "bw", "per_cu") == (4 * (12288 + 344) + 2048, 12288, 3)  # 52,576
    # counters beside the bitmap only when n of them fit it: (3,6) 2 n <= 3 n; dv = 1: 2 n > n
    assert f(R(10000, 3, 6), "fb", "fbu", "emit_fb") == (2, 2, -1)
    assert f(R(8192, 1, 2), "fb", "fbu", "emit_fb") == (2, 0, -1)
    # no variable-side kernel: the emit pass counts in LDS (fbu) or claims by global CAS (0)
    assert f(R(60, 255, 3), "fbu", "emit_fb", "vs_lds") == (8, 8, 0)
    assert f(C(6000, 4000, 12000, 3, 256), "fbu", "emit_fb", "vs_lds") == (0, 0, 0)
    # variable-side LDS: V fb / 8 bytes of counters, then the rows
    assert f(R(24576, 3, 6), "vs_lds") == (24576 * 2 // 8 + 2 * 24576 * 3,)  # 153,600
    assert f(C(6000, 4000, 12000, 3, 255), "vs_lds") == (256 + 2 * 256 * 255,)


def test_reciprocal_of_dv():
    def mdv(n, dv, dc):
        return sample_plan(*R(n, dv, dc))["mdv"]
    assert mdv(8192, 1, 2) == 0 and mdv(4096, 2, 4) == 1 << 31 and mdv(2731, 3, 3) == 1431655766
    assert mdv(60, 255, 3) == 16843010 == -(-(1 << 32) // 255) and mdv(60, 256, 3) == 0
    assert sample_plan(*C(6000, 4000, 12000, 3, 3))["mdv"] == 0  # irregular: a table lookup, no division


@pytest.mark.parametrize("shape,per_cu", [(R(131072, 3, 6), 3), (R(21846, 3, 6), 15), (R(4096, 2, 4), 32)])
def test_search_grid_on_both_sides_of_the_device(shape, per_cu):
    """W = min(G, cus per_cu): 160 KiB / LDS workgroups per CU, at most 32; no device, no search."""
    for cus in (256, 304):
        cap = cus * per_cu
        for G in (1, cap - 1, cap, cap + 1, 4 * cap):
            p = sample_plan(*shape[:7], G, cus)
            assert (p["per_cu"], p["W"]) == (per_cu, min(G, cap)) and p["search"].startswith("sample_search_kernel<")
    p = sample_plan(*shape[:7], 6, 0)
    assert (p["per_cu"], p["W"], p["search"]) == (0, 0, "none")


def test_sweep_invariants():
    """Over a few thousand shapes: the sequential sampler exactly inside its window; LDS within a
    CU's 160 KiB; the bitmap covers E; a 16-bit ring, permutation or row only where every id
    fits; counters wide enough for the largest degree; whole waves of variables per chunk."""
    plans = u.sweep_plans()
    assert len(plans) > 3000
    for s, p in plans:
        n, m, E, cdeg, vdeg, regular, dv, G, cus = s
        assert p["seq"] == (8192 <= E <= 393216 and cdeg <= 192), s
        assert 0 < p["lds"] <= 160 * 1024 and p["vs_lds"] <= 160 * 1024, (s, p)
        if not p["seq"]:
            assert p["threads"] == p["K"] and p["W"] == p["V"] == p["bw"] == 0, (s, p)
            if p["draw"] != ONE1024:  # u16 permutation in LDS
                assert n <= 65536 and E < 65536 and p["K"] == (256 if E <= 16384 else 512), (s, p)
                assert p["draw"] == (ONE256 if p["K"] == 256 else ONE512), (s, p)
            else:
                assert (n > 65536 or E >= 65536) and p["lds"] == 65600, (s, p)
            continue
        assert p["threads"] == 128 and p["K"] == 0, (s, p)
        assert p["bw"] % 4 == 0 and 32 * p["bw"] >= E > 32 * (p["bw"] - 4), (s, p)
        assert p["ring"] == (2 if n <= 65536 else 4), (s, p)
        assert p["draw"] == {(True, 2): SEQ_RU, (True, 4): SEQ_RI, (False, 2): SEQ_CU, (False, 4): SEQ_CI}[regular, p["ring"]]
        assert p["fb"] in (0, 2, 4, 8) and (vdeg < (1 << p["fb"]) if p["fb"] else vdeg >= 256), (s, p)
        assert p["fbu"] in (0, p["fb"]) and (p["fbu"] == 0 or n * p["fbu"] <= 32 * p["bw"]), (s, p)
        assert p["row"] == (2 if (m if regular else E) <= 65536 else 4), (s, p)
        assert p["V"] % 64 == 0 and p["V"] <= n and (p["V"] > 0) == (p["fb"] > 0 and n >= 64), (s, p)
        assert p["emit_fb"] == (-1 if p["V"] else p["fbu"]), (s, p)
        if p["V"]:
            assert p["nch"] == -(-n // p["V"]) and p["vs_lds"] == p["V"] * p["fb"] // 8 + p["row"] * p["V"] * vdeg, (s, p)
            assert p["var_side"] == (VS16 if p["row"] == 2 else VS32), (s, p)
        else:
            assert (p["nch"], p["vs_lds"], p["var_side"]) == (0, 0, "none"), (s, p)
        if cus:
            assert p["per_cu"] == max(1, min(32, 160 * 1024 // p["lds"])) and p["W"] == min(G, cus * p["per_cu"]), (s, p)
        else:
            assert (p["W"], p["per_cu"], p["search"]) == (0, 0, "none"), (s, p)
    assert u.sweep_names() == {ONE256, ONE512, ONE1024, SEQ_RU, SEQ_RI, SEQ_CU, SEQ_CI, VS16, VS32} | {
        f"sample_search_kernel<{a},{b}>" for a in ("regular", "csr") for b in ("u16", "int")}
