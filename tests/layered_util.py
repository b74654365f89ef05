"""Graphs, schedules and launch plans the layered-schedule tests share."""
import functools

import numpy as np

from tests.graph_util import FALLBACK_KERNELS, csr_from_checks, fallback_csr, regular_simple

KEYS = ("path", "threads", "grid", "lds", "lds_slots", "persistent", "slab", "counter", "scratch")
LDS_CAP = 160 * 1024 - 4096  # the budget of the block's LDS words and the Monte-Carlo curve (gmem_plan's)


@functools.lru_cache(maxsize=None)
def graph_csr(name):
    """CSR slot form of "r36_<n>" (regular_simple(n, 3, 6, seed=1)) or a FALLBACK_KERNELS name."""
    if name in FALLBACK_KERNELS:
        return fallback_csr(name)
    kind, n = name.split("_")
    assert kind == "r36"
    g = regular_simple(int(n), 3, 6, seed=1)
    return csr_from_checks(np.arange(g.m + 1) * 6, g.check_lookup, g.n)


@functools.lru_cache(maxsize=None)
def graph(name):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    return TannerGraph.from_csr(*graph_csr(name))


def schedule(csr):
    """(rc, number of layers, layer of every check) of ldpc_debug_layer_schedule (host only)."""
    import ctypes as ct
    from iib_project_ldpc_codes_amd import _native
    cptr, cvar, vptr, vslot = [np.ascontiguousarray(a, np.int32) for a in csr]
    num = ct.c_int32(-1)
    layer = np.full(cptr.size - 1, -1, np.int32)
    rc = _native.lib().ldpc_debug_layer_schedule(cptr.ctypes.data, cvar.ctypes.data, vptr.ctypes.data,
                                                 vslot.ctypes.data, vptr.size - 1, cptr.size - 1, ct.addressof(num),
                                                 layer.ctypes.data)
    return rc, num.value, layer


@functools.lru_cache(maxsize=None)
def layers(name):
    rc, L, layer = schedule(graph_csr(name))
    assert rc == 0
    layer.setflags(write=False)
    return L, layer


def layer_plans(csr, calls, cus=256):
    """bp_layer_plan (ldpc_debug_layer_plan, host only) of `calls` = (algo, early_stop, mc,
    want_post, iters, B) tuples on one CSR graph, as graph_util.bp_plans."""
    from iib_project_ldpc_codes_amd import _native
    cptr, cvar, vptr, vslot = [np.ascontiguousarray(a, np.int32) for a in csr]
    args = np.ascontiguousarray([[B, iters, algo, es, mc, post] for algo, es, mc, post, iters, B in calls], np.int32)
    out = np.zeros((len(calls), 9), np.int64)
    names = np.zeros((len(calls), 64), np.uint8)
    rc = _native.lib().ldpc_debug_layer_plan(cptr.ctypes.data, cvar.ctypes.data, vptr.ctypes.data, vslot.ctypes.data,
                                             vptr.size - 1, cptr.size - 1, len(calls), args.ctypes.data, cus,
                                             out.ctypes.data, names.ctypes.data)
    assert rc == 0, _native.last_error()
    plans = [dict(zip(KEYS, (int(x) for x in row))) for row in out]
    for p, nm in zip(plans, names):
        p["name"] = nm.tobytes().split(b"\0")[0].decode()
    return plans


def kernel_name(csr, lds):
    """The display name bp_layer_plan must give a graph: width by the largest check degree."""
    d = int(np.diff(csr[0]).max())
    return "bp_layer_kernel<%d,%s>" % (8 if d <= 8 else 16 if d <= 16 else 32, "lds" if lds else "gmem")
