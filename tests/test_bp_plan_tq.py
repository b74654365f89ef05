"""Host-only: the compile-time width of the soft decoders' plans (BpPlan::tq, through ldpc_debug_bp_plan_tq).

The fixed-count sum-product call on a chained layout whose Tq = n / 20 is listed in LDPC_LOC_CHAIN_TQ
(kernel_shapes.hpp: 500, n = 10,000) runs bp_loc_chain_kernel<5, 512, TQ=500>, whose row offsets are instruction
immediates; the launcher starts that instantiation on a plan that names it and on no other.  Every other width
(205 at n = 4,100), every other mode, a graph on the plain layout, and every call of a graph built under
LDPC_NO_LOC_TQ=1 (read with the other layout switches, each time a graph's layouts are built) plan 0: the generic
instantiation.  The launch width and ldpc_debug_bp_plan's nine fields do not depend on it.
"""
import functools
import os

import numpy as np
import pytest

from iib_project_ldpc_codes_amd import _native
from iib_project_ldpc_codes_amd.graph import TannerGraph
from tests.graph_util import bp_plans, csr_from_checks

# (algo, early_stop, mc, want_post, iters, B): the chained call first (with and without posteriors), then min-sum,
# early stop with and without posteriors, Monte-Carlo with and without early stop
CALLS = [(0, 0, 0, 1, 50, 300), (0, 0, 0, 0, 7, 3), (1, 0, 0, 1, 50, 300), (0, 1, 0, 1, 50, 300), (0, 1, 0, 0, 50, 300),
         (0, 0, 1, 0, 50, 300), (0, 1, 1, 0, 50, 300), (1, 1, 0, 0, 50, 300), (1, 0, 1, 0, 50, 300)]
CHAINED = 2  # the first two calls take the chained layout
SWITCHES = ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T", "LDPC_NO_LOC_CHAIN", "LDPC_NO_LOC_TQ")


@functools.lru_cache(maxsize=None)
def csr_of(n):
    g = TannerGraph.random_regular(n, 3, 6, seed=1)
    return csr_from_checks(np.arange(g.m + 1) * 6, np.ascontiguousarray(g.check_lookup, np.int32), g.n)


def plan_ints(entry, csr, calls, cus=256):
    cptr, cvar, vptr, vslot = csr
    args = np.ascontiguousarray([[B, iters, algo, es, mc, post] for algo, es, mc, post, iters, B in calls], np.int32)
    out = np.full(len(calls), -1, np.int64)
    rc = getattr(_native.lib(), entry)(cptr.ctypes.data, cvar.ctypes.data, vptr.ctypes.data, vslot.ctypes.data,
                                       vptr.size - 1, cptr.size - 1, len(calls), args.ctypes.data, cus, out.ctypes.data)
    assert rc == 0, _native.last_error()
    return [int(w) for w in out]


@pytest.fixture
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_bench_code_plans_its_width(clean_env):
    csr = csr_of(10000)
    tq, width = plan_ints("ldpc_debug_bp_plan_tq", csr, CALLS), plan_ints("ldpc_debug_bp_plan_width", csr, CALLS)
    assert tq == [500] * CHAINED + [0] * (len(CALLS) - CHAINED)
    assert width[:CHAINED] == [500] * CHAINED and all(w == 512 for w in width[CHAINED:])
    plans = bp_plans(csr, CALLS)
    # the switch: the same plans but for tq
    clean_env.setenv("LDPC_NO_LOC_TQ", "1")
    assert plan_ints("ldpc_debug_bp_plan_tq", csr, CALLS) == [0] * len(CALLS)
    assert plan_ints("ldpc_debug_bp_plan_width", csr, CALLS) == width
    clean_env.setenv("LDPC_NO_LOC_TQ", "0")  # only "1" switches it off, as the other layout switches
    assert plan_ints("ldpc_debug_bp_plan_tq", csr, CALLS) == tq
    clean_env.delenv("LDPC_NO_LOC_TQ")
    assert bp_plans(csr, CALLS, env={"LDPC_NO_LOC_TQ": "1"}) == plans
    os.environ.pop("LDPC_NO_LOC_TQ", None)  # bp_plans leaves its env behind
    assert plan_ints("ldpc_debug_bp_plan_tq", csr, CALLS) == tq


def test_unlisted_width_plans_the_generic_instantiation(clean_env):
    csr = csr_of(4100)
    assert plan_ints("ldpc_debug_bp_plan_width", csr, CALLS)[:CHAINED] == [205] * CHAINED  # chained, Tq = 205
    assert plan_ints("ldpc_debug_bp_plan_tq", csr, CALLS) == [0] * len(CALLS)


def test_plain_layout_plans_none(clean_env):
    """A graph without a chained layout (P no multiple of 5), and the bench code with the chained layout off."""
    csr = csr_of(4104)
    assert all(p["name"] == "bp_loc_kernel" for p in bp_plans(csr, CALLS[:CHAINED]))
    assert plan_ints("ldpc_debug_bp_plan_width", csr, CALLS[:CHAINED]) == [512] * CHAINED
    assert plan_ints("ldpc_debug_bp_plan_tq", csr, CALLS) == [0] * len(CALLS)
    clean_env.setenv("LDPC_NO_LOC_CHAIN", "1")
    csr = csr_of(10000)
    assert plan_ints("ldpc_debug_bp_plan_width", csr, CALLS[:CHAINED]) == [512] * CHAINED
    assert plan_ints("ldpc_debug_bp_plan_tq", csr, CALLS) == [0] * len(CALLS)


def test_bad_arguments_are_refused():
    cptr, cvar, vptr, vslot = csr_of(4100)
    out = np.zeros(1, np.int64)
    calls = np.array([[300, 50, 0, 0, 0, 1]], np.int32)
    ptrs = (cptr.ctypes.data, cvar.ctypes.data, vptr.ctypes.data, vslot.ctypes.data, vptr.size - 1, cptr.size - 1)
    lib = _native.lib()
    assert lib.ldpc_debug_bp_plan_tq(*ptrs, 1, calls.ctypes.data, 0, out.ctypes.data) == _native.LDPC_EINVAL
    assert lib.ldpc_debug_bp_plan_tq(*ptrs, 1, None, 256, out.ctypes.data) == _native.LDPC_EINVAL
    assert lib.ldpc_debug_bp_plan_tq(*ptrs, 1, calls.ctypes.data, 256, None) == _native.LDPC_EINVAL
    assert lib.ldpc_debug_bp_plan_tq(*ptrs, 0, None, 256, None) == _native.LDPC_OK
