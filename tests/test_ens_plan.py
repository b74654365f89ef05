"""Host-only checks of the ensemble soft decoder's launch plan (csrc/bp_plan.cpp bp_ens_plan)
through ldpc_debug_ens_plan, no device needed: which bp_ens_kernel instantiation a call runs and
its grid, LDS and slab layout.

One workgroup owns one block of pad16(8 E + 4 n) bytes, E = n dv (messages float[E], channel
LLRs float[n], cross index int32[E]): in LDS when it fits under 160 KiB - 2 KiB beside the
early-stop syndrome bits (two buffers of one bit per check, 16-byte padded) and the Monte-Carlo
curve (4 (iters + 1) bytes), else one slab of scratch per workgroup, with the first lds_slots
messages in the LDS left beside the (16-byte padded) curve and the syndrome bits.
"""
import numpy as np
import pytest

from iib_project_ldpc_codes_amd import _native
from tests.graph_util import bp_plans, csr_from_checks, regular_simple

KIB = 1024
KEYS = ("path", "threads", "grid", "lds", "lds_slots", "persistent", "slab", "counter", "scratch")


def ens_plans(n, dv, dc, calls, cus=256):
    """(rc, plans) of `calls` = (algo, early_stop, mc, want_post, iters, B) tuples, the call
    format of tests.graph_util.bp_plans."""
    args = np.ascontiguousarray([[B, iters, algo, es, mc, post] for algo, es, mc, post, iters, B in calls], np.int32)
    out = np.zeros((len(calls), 9), np.int64)
    names = np.zeros((len(calls), 64), np.uint8)
    rc = _native.lib().ldpc_debug_ens_plan(n, dv, dc, len(calls), args.ctypes.data, cus, out.ctypes.data,
                                           names.ctypes.data)
    plans = [dict(zip(KEYS, (int(x) for x in row))) for row in out]
    for p, nm in zip(plans, names):
        p["name"] = nm.tobytes().split(b"\0")[0].decode()
    return rc, plans


def block_bytes(n, dv):
    return (8 * n * dv + 4 * n + 15) & ~15


def syn_bytes(n, dv, dc):
    return (2 * 4 * ((n * dv // dc + 31) // 32) + 15) & ~15


MODES = [(algo, es, mc, post) for algo in (0, 1) for es in (0, 1) for mc in (0, 1) for post in (0, 1)]


@pytest.mark.parametrize("n,dv,dc,name", [(200, 3, 6, "bp_ens_kernel<8,lds>"), (90, 3, 9, "bp_ens_kernel<16,lds>"),
                                          (96, 3, 8, "bp_ens_kernel<8,lds>"), (160, 3, 16, "bp_ens_kernel<16,lds>"),
                                          (170, 3, 17, "bp_ens_kernel<32,lds>"), (320, 3, 32, "bp_ens_kernel<32,lds>")])
def test_small_shapes_decode_in_lds(n, dv, dc, name):
    calls = [m + (it, B) for m in MODES for it in (0, 1, 20) for B in (1, 48, 264)]
    rc, plans = ens_plans(n, dv, dc, calls)
    assert rc == 0, _native.last_error()
    for call, p in zip(calls, plans):
        mc, iters, B = call[2], call[4], call[5]
        assert p["name"] == name, (call, p)
        assert p["threads"] == 256 and p["grid"] == min(B, 256), (call, p)
        assert p["lds"] == block_bytes(n, dv) + syn_bytes(n, dv, dc) + (4 * (iters + 1) if mc else 0), (call, p)
        assert p["slab"] == p["scratch"] == p["lds_slots"] == 0 and p["counter"] == -1 and not p["persistent"], (call, p)


@pytest.mark.parametrize("n", [10000, 64800])
def test_36_large_shapes_decode_on_slabs(n):
    E = 3 * n
    calls = [m + (it, B) for m in MODES for it in (1, 50) for B in (1, 6, 300, 70000)]
    rc, plans = ens_plans(n, 3, 6, calls)
    assert rc == 0, _native.last_error()
    for call, p in zip(calls, plans):
        mc, iters, B = call[2], call[4], call[5]
        assert p["name"] == "bp_ens_kernel<8,gmem>", (call, p)
        assert p["threads"] == 1024 and p["grid"] == min(B, 256), (call, p)
        assert p["slab"] == p["scratch"] == p["grid"] * block_bytes(n, 3), (call, p)
        fixed = ((4 * (iters + 1) + 15) & ~15 if mc else 0) + syn_bytes(n, 3, 6)
        assert p["lds_slots"] == min(E, (160 * KIB - 4096 - fixed) // 4), (call, p)
        assert p["lds"] == fixed + 4 * p["lds_slots"] <= 160 * KIB - 4096, (call, p)
        assert p["counter"] == -1 and not p["persistent"], (call, p)
    # n = 10,000: every message in LDS (the slab keeps the LLRs and the index);
    # n = 64,800: most messages in the slab
    assert all((p["lds_slots"] == E) == (n == 10000) for p in plans)


def test_curve_bytes_push_a_near_limit_shape_off_lds():
    """(3,6) n = 5,700: block and syndrome bits take 159,600 + 720 bytes, 1,472 under the LDS budget
    of 160 KiB - 2 KiB; a Monte-Carlo curve of up to 368 entries fits beside them, a longer one
    does not.  A plain decode has no curve and stays in LDS at any iteration count."""
    n, budget = 5700, 160 * KIB - 2048
    room = budget - block_bytes(n, 3) - syn_bytes(n, 3, 6)
    assert room == 1472
    last_fit = room // 4 - 1  # iterations whose curve of iters + 1 entries just fits
    calls = [(1, 1, 1, 0, 50, 64), (1, 1, 1, 0, last_fit, 64), (1, 1, 1, 0, last_fit + 1, 64), (1, 1, 1, 0, 5000, 64),
             (1, 1, 0, 1, 5000, 64)]
    rc, plans = ens_plans(n, 3, 6, calls)
    assert rc == 0, _native.last_error()
    assert [p["name"].split(",")[1] for p in plans] == ["lds>", "lds>", "gmem>", "gmem>", "lds>"]
    assert plans[1]["lds"] == budget and plans[1]["scratch"] == 0
    for p in plans[2:4]:
        assert p["scratch"] == 64 * block_bytes(n, 3) and p["lds"] <= 160 * KIB - 4096


def test_check_degree_above_32_is_unsupported():
    rc, plans = ens_plans(330, 3, 33, [(0, 0, 0, 1, 20, 8), (1, 1, 1, 0, 20, 8)])
    assert rc == _native.LDPC_EUNSUP
    assert all(p["name"] == "none" and p["grid"] == 0 and p["scratch"] == 0 for p in plans)
    assert "32" in _native.last_error()
    rc, _ = ens_plans(330, 3, 30, [(0, 0, 0, 1, 20, 8)])
    assert rc == 0
    rc, _ = ens_plans(200, 3, 7, [(0, 0, 0, 1, 20, 8)])  # n dv not divisible by dc
    assert rc == _native.LDPC_EINVAL


@pytest.mark.parametrize("n,dv,dc", [(200, 3, 6), (90, 3, 9), (10000, 3, 6), (64800, 3, 6), (1000, 5, 10)])
def test_grid_never_exceeds_the_batch_or_the_cus(n, dv, dc):
    calls = [(1, 1, mc, 0, 20, B) for mc in (0, 1) for B in (1, 2, 7, 255, 256, 257, 4096)]
    for cus in (8, 256, 304):
        rc, plans = ens_plans(n, dv, dc, calls, cus=cus)
        assert rc == 0
        for call, p in zip(calls, plans):
            assert 1 <= p["grid"] == min(call[5], cus, 256), (cus, call, p)
            assert p["scratch"] == p["slab"] and p["slab"] % p["grid"] == 0, (cus, call, p)
            assert p["lds"] <= 160 * KIB and p["threads"] in (256, 1024), (cus, call, p)


def test_plans_of_prepared_graphs_are_unchanged():
    """bp_ens_plan is a function of its own: the same calls on one fixed (3,6) graph plan the
    same before and after ensemble plans were asked for, and never name the ensemble kernel."""
    g = regular_simple(1000, 3, 6, seed=1)
    csr = csr_from_checks(np.arange(g.m + 1) * 6, g.check_lookup, g.n)
    calls = [m + (it, B) for m in MODES for it in (0, 50) for B in (1, 300)]
    before = bp_plans(csr, calls)
    rc, ens = ens_plans(1000, 3, 6, calls)
    assert rc == 0
    assert bp_plans(csr, calls) == before
    assert not any("ens" in p["name"] for p in before) and all("bp_ens_kernel" in p["name"] for p in ens)
