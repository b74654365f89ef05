"""Host-only: the launch width of the soft decoders' plans (BpPlan::width, through ldpc_debug_bp_plan_width).

The fixed-count sum-product call on a graph with a chained layout launches that layout's Tq = n / 20 threads
(bp_loc_chain_kernel strides by its launch width and tests no lane): 205, 500 and 510 at n = 4,100 (a
part-filled last wave, four waves that are never started), 10,000 (the bench code) and 10,200 (the largest that
fits).  Every other mode, and every mode under LDPC_NO_LOC_CHAIN=1, launches the plan's `threads`.  The nine
fields ldpc_debug_bp_plan reports do not move: `threads` stays 512 for the chained call, and each field equals
what the plain layout's plan says but `lds`, whose value is the chained layout's message words.
"""
import functools
import os

import numpy as np
import pytest

from iib_project_ldpc_codes_amd import _native
from iib_project_ldpc_codes_amd.graph import TannerGraph
from tests.graph_util import bp_plans, csr_from_checks

# (algo, early_stop, mc, want_post, iters, B): the chained call first, then min-sum, early stop with and without
# posteriors, Monte-Carlo with and without early stop
CALLS = [(0, 0, 0, 1, 50, 300), (1, 0, 0, 1, 50, 300), (0, 1, 0, 1, 50, 300), (0, 1, 0, 0, 50, 300),
         (0, 0, 1, 0, 50, 300), (0, 1, 1, 0, 50, 300), (1, 1, 0, 0, 50, 300), (1, 0, 1, 0, 50, 300)]
TQ = {4100: 205, 10000: 500, 10200: 510}


@functools.lru_cache(maxsize=None)
def csr_of(n):
    g = TannerGraph.random_regular(n, 3, 6, seed=1)
    return csr_from_checks(np.arange(g.m + 1) * 6, np.ascontiguousarray(g.check_lookup, np.int32), g.n)


def widths(csr, calls, cus=256):
    cptr, cvar, vptr, vslot = csr
    args = np.ascontiguousarray([[B, iters, algo, es, mc, post] for algo, es, mc, post, iters, B in calls], np.int32)
    out = np.full(len(calls), -1, np.int64)
    saved = {k: os.environ.pop(k, None) for k in ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T")}
    try:
        rc = _native.lib().ldpc_debug_bp_plan_width(cptr.ctypes.data, cvar.ctypes.data, vptr.ctypes.data,
                                                    vslot.ctypes.data, vptr.size - 1, cptr.size - 1, len(calls),
                                                    args.ctypes.data, cus, out.ctypes.data)
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    assert rc == 0, _native.last_error()
    return [int(w) for w in out]


@pytest.mark.parametrize("n", sorted(TQ))
def test_chained_call_launches_tq_threads(monkeypatch, n):
    csr = csr_of(n)
    monkeypatch.delenv("LDPC_NO_LOC_CHAIN", raising=False)
    on, w_on = bp_plans(csr, CALLS), widths(csr, CALLS)
    monkeypatch.setenv("LDPC_NO_LOC_CHAIN", "1")
    off, w_off = bp_plans(csr, CALLS), widths(csr, CALLS)
    assert all(p["name"] == "bp_loc_kernel" and p["threads"] == 512 for p in (on[0], off[0]))
    assert w_on[0] == TQ[n] == n // 20
    # every other mode, and every mode without the chained layout, launches `threads`
    assert w_on[1:] == [p["threads"] for p in on[1:]]
    assert w_off == [p["threads"] for p in off]
    assert all(w > 0 for w in w_on + w_off)
    # the nine fields are what they were: the plain layout's but for the chained call's lds
    assert on[1:] == off[1:]
    assert {k: v for k, v in on[0].items() if k != "lds"} == {k: v for k, v in off[0].items() if k != "lds"}
    # message words: 32 Tq on the chained layout, E - n = 2 n on the plain one, 64 spare words behind either
    assert on[0]["lds"] == 4 * (32 * TQ[n] + 64) and off[0]["lds"] == 4 * (2 * n + 64)


def test_width_is_threads_on_the_other_paths(monkeypatch):
    """Graphs without a chained layout (P no multiple of 5; no local-edge layout at all) on every mode."""
    monkeypatch.delenv("LDPC_NO_LOC_CHAIN", raising=False)
    for n in (4104, 1000):
        csr = csr_of(n)
        assert widths(csr, CALLS) == [p["threads"] for p in bp_plans(csr, CALLS)]


def test_bad_arguments_are_refused():
    csr = csr_of(4100)
    cptr, cvar, vptr, vslot = csr
    out = np.zeros(1, np.int64)
    calls = np.array([[300, 50, 0, 0, 0, 1]], np.int32)
    ptrs = (cptr.ctypes.data, cvar.ctypes.data, vptr.ctypes.data, vslot.ctypes.data, vptr.size - 1, cptr.size - 1)
    lib = _native.lib()
    assert lib.ldpc_debug_bp_plan_width(*ptrs, 1, calls.ctypes.data, 0, out.ctypes.data) == _native.LDPC_EINVAL
    assert lib.ldpc_debug_bp_plan_width(*ptrs, 1, None, 256, out.ctypes.data) == _native.LDPC_EINVAL
    assert lib.ldpc_debug_bp_plan_width(*ptrs, 1, calls.ctypes.data, 256, None) == _native.LDPC_EINVAL
    assert lib.ldpc_debug_bp_plan_width(*ptrs, 0, None, 256, None) == _native.LDPC_OK
