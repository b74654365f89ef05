"""What the Gallager A/B tests share: the launch plan's rows (ldpc_debug_gb_plan, host only), the graphs,
the oracle's BSC words and the reference's answers, each computed once and kept read-only."""
import functools

import numpy as np

from tests import gallager_ref as ref
from tests.layered_util import graph, graph_csr  # noqa: F401  (graph: one TannerGraph per name)

PLAN_KEYS = ("threads", "W", "plane", "cw_per_wg", "grid", "lds", "cap", "scratch")
LDS_CAP = 160 * 1024 - 4096
SEED = 11

# (graph, b) -> crossover probability at which, of the 256 trials 0 .. 255 of the oracle's BSC stream
# under SEED, at least 8 stop early within 20 iterations and at least 8 run to the cap.  Found by
# scanning the reference alone (the issue's table for the rows it lists, the same scan for the others);
# every early-stop and Monte-Carlo test asserts the condition on the reference before it looks at the
# device (assert_stop_mix).  (stopped early, at the cap) of that scan is noted where the issue has no row.
P_MIX = {
    ("r36_600", 0): 0.03, ("r36_600", 1): 0.005, ("r36_600", 2): 0.03,      # b = 1: 234 / 22
    ("r36_602", 0): 0.03, ("r36_602", 1): 0.005, ("r36_602", 2): 0.03,      # b = 1: 232 / 24
    ("r48_256", 0): 0.03, ("r48_256", 1): 0.03, ("r48_256", 2): 0.01, ("r48_256", 3): 0.03,  # b = 1: 203 / 53
    # b = 0 and 4: 209 / 47, b = 1: 200 / 56, b = 2: 221 / 35
    ("r510_640", 0): 0.02, ("r510_640", 1): 0.02, ("r510_640", 2): 0.007, ("r510_640", 3): 0.02, ("r510_640", 4): 0.02,
    ("mixA", 0): 0.03, ("mixA", 1): 0.005, ("mixA", 2): 0.02, ("mixA", 3): 0.03,  # b = 1: 208 / 48
    ("mixB", 0): 0.003, ("mixB", 1): 0.003, ("mixB", 2): 0.003,             # 149 / 107 (0.01: 9 / 247)
    ("r36_10000", 0): 0.038,
}
EXTRA_B = {"r510_640": (3,)}  # the issue's table has this row beside 0, 1, 2 and dv - 1


def shape(name):
    """(n, E, largest variable degree) of a graph."""
    csr = graph_csr(name)
    return csr[2].size - 1, csr[1].size, int(np.diff(csr[2]).max())


def b_values(name):
    """The flip thresholds the tests run a graph at: 0, 1, 2 and dv - 1 (the largest degree's)."""
    return sorted({0, 1, 2, shape(name)[2] - 1} | set(EXTRA_B.get(name, ())))


def gb_plans(n, E, calls):
    """gb_plan's rows of `calls` = (B, iters, early_stop, mc) tuples on a graph of n variables and E slots."""
    from iib_project_ldpc_codes_amd import _native
    args = np.ascontiguousarray(calls, np.int32).reshape(len(calls), 4)
    out = np.zeros((len(calls), 8), np.int64)
    names = np.zeros((len(calls), 64), np.uint8)
    rc = _native.lib().ldpc_debug_gb_plan(n, E, len(calls), args.ctypes.data, out.ctypes.data, names.ctypes.data)
    assert rc == 0, _native.last_error()
    plans = [dict(zip(PLAN_KEYS, (int(x) for x in row))) for row in out]
    for p, nm in zip(plans, names):
        p["name"] = nm.tobytes().split(b"\0")[0].decode()
    return plans


def plan(name, B, iters, early_stop, mc):
    n, E, _ = shape(name)
    return gb_plans(n, E, [(B, iters, int(early_stop), int(mc))])[0]


@functools.lru_cache(maxsize=None)
def bsc_bits(name, p, seed, first, B):
    """Received words of trials first .. first + B - 1: 1 where the oracle's BSC LLR is negative."""
    from oracle import oracle
    from tests import index64_util as u
    n = shape(name)[0]
    y = (u.channel_rows(oracle.CH_BSC, p, seed, u.true_indices(first, B), n) < 0).astype(np.uint8)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def decoded(name, p, seed, first, B, iters, b, early_stop):
    """(hard, its, curve) of the reference on bsc_bits(name, p, seed, first, B)."""
    out = ref.decode(graph_csr(name), bsc_bits(name, p, seed, first, B), iters, b, early_stop)
    for a in out:
        a.setflags(write=False)
    return out


def stop_mix(its, cap):
    """(frames stopped before the cap, frames at the cap)."""
    its = np.asarray(its)
    return int((its < cap).sum()), int((its == cap).sum())


def assert_stop_mix(its, cap):
    early, at_cap = stop_mix(its, cap)
    assert early >= 8 and at_cap >= 8, "the case does not exercise early stop: %d early, %d at the cap" % (early, at_cap)
