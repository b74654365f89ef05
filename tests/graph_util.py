"""Test graphs that the ensembles module does not draw."""
import numpy as np


def check6_var24(m, seed=0):
    """Check-regular degree-6 rate-1/2 graph with variable degrees {2, 4}: n = 2m, variables
    0..m-1 of degree 2 on a ring (variable i joins checks i and i+1 mod m, so every check can
    take a degree-2 variable as its slot-0 local edge), variables m..2m-1 of degree 4 on
    random checks (4 sockets per check, no repeated check per variable).  Its local-edge
    layout has every check at degree 6 but DVN = 3 -- the shape that must run on the RSU
    instantiation of bp_loc_kernel, not the (3,6) one (advisor round 2)."""
    from iib_project_ldpc_codes_amd.ensembles import _csr_from_pairs
    rng = np.random.default_rng(seed)
    sock = np.repeat(np.arange(m), 4)
    rng.shuffle(sock)
    rows = sock.reshape(m, 4)
    for _ in range(1000):
        bad = [j for j in range(m) if len(set(rows[j])) < 4]
        if not bad:
            break
        for j in bad:  # swap one socket of the offending variable with a random socket
            a, b = rng.integers(4), rng.integers(m)
            c = rng.integers(4)
            rows[j, a], rows[b, c] = rows[b, c], rows[j, a]
    assert all(len(set(r)) == 4 for r in rows)
    pairs = [(i, i) for i in range(m)] + [(i, (i + 1) % m) for i in range(m)]
    pairs += [(m + j, int(c)) for j in range(m) for c in rows[j]]
    return _csr_from_pairs(2 * m, m, np.full(m, 6, np.int32), pairs)


def regular_simple(n, dv, dc, seed=0):
    """A (dv, dc)-regular graph without repeated edges in the reference's list format, for
    degrees where TannerGraph.random_regular's whole-graph redraw almost never succeeds: one
    uniform socket permutation, then every slot that repeats a variable in its check swaps
    variables with a random slot until none is left (not the configuration model's law)."""
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    rng = np.random.default_rng(seed)
    E, m = n * dv, n * dv // dc
    assert m * dc == E
    chk = np.arange(E) // dc
    cvar = np.repeat(np.arange(n, dtype=np.int32), dv)[rng.permutation(E)]
    for _ in range(1000):
        key = chk.astype(np.int64) * n + cvar
        order = np.argsort(key, kind="stable")
        dup = order[1:][key[order][1:] == key[order][:-1]]
        if not dup.size:
            break
        for s in dup:
            t = rng.integers(E)
            cvar[s], cvar[t] = cvar[t], cvar[s]
    else:
        raise RuntimeError("regular_simple: repeated edges left")
    var = chk[np.lexsort((chk, cvar))].astype(np.int32)  # by variable, then ascending check
    return TannerGraph(var, cvar, n, n - m, dv, dc)


def mixed_checks(degrees, n, seed=0):
    """A graph whose check c has degree degrees[c] (any multiset, every degree >= 2) on n
    variables, as (check_ptr, check_var): the sum(degrees) sockets are dealt to the variables as
    evenly as they divide (variable degrees floor / ceil of E / n) by one uniform socket
    permutation, then every slot that repeats a variable in its check swaps variables with a
    random slot until none is left, as regular_simple does."""
    rng = np.random.default_rng(seed)
    degrees = np.asarray(degrees, np.int64)
    assert degrees.min() >= 2 and degrees.max() <= n
    cptr = np.concatenate(([0], np.cumsum(degrees)))
    E = int(cptr[-1])
    assert E >= n
    chk = np.repeat(np.arange(degrees.size), degrees)
    cvar = (np.arange(E, dtype=np.int32) % n)[rng.permutation(E)]
    for _ in range(1000):
        key = chk.astype(np.int64) * n + cvar
        order = np.argsort(key, kind="stable")
        dup = order[1:][key[order][1:] == key[order][:-1]]
        if not dup.size:
            break
        for s in dup:
            t = rng.integers(E)
            cvar[s], cvar[t] = cvar[t], cvar[s]
    else:
        raise RuntimeError("mixed_checks: repeated edges left")
    return cptr.astype(np.int32), cvar


def extreme_llrs(n, B, seed):
    """BI-AWGN LLRs with the values at the edges of fp32 that a kernel can mishandle mixed in:
    0 and -0, +-1e-30, +-1e4, +-1e30 (beyond the kernels' staging clamp)."""
    from oracle import oracle
    rs = np.random.RandomState(seed)
    llr = oracle.channel(oracle.CH_AWGN, 0.80, seed, 0, n, B)
    sign = np.where(rs.rand(B, n) < 0.5, -1.0, 1.0).astype(np.float32)
    u = rs.rand(B, n)
    llr = np.where(u < 0.08, 0.0, llr)
    llr = np.where((u >= 0.08) & (u < 0.10), sign * 1e-30, llr)
    llr = np.where((u >= 0.10) & (u < 0.14), sign * 1e4, llr)
    llr = np.where((u >= 0.14) & (u < 0.16), sign * 1e30, llr)
    llr[:, 0] = -0.0
    return np.ascontiguousarray(llr, np.float32)


# Graphs off the headline path: name -> the kernel a plain 20-iteration decode of 24 frames runs
# (tests/test_bp_plan.py and tests/test_gpu_fallback.py hold the plan to these names).
# r<dv><dc>_<n> is regular_simple(n, dv, dc, seed=1); mixA / mixB are mixed_checks graphs.
FALLBACK_KERNELS = {
    "r48_256": "bp_irr_kernel<lds>",            # DC = 8, every message in LDS
    "r48_9216": "bp_irr_kernel<lds+slab>",      # DC = 8, rows beyond LDS in the slab
    "r58_320": "bp_generic_kernel<8,lds>",      # variable degree 5 > kFloodDV: the looped variable branch
    "r58_8800": "bp_generic_kernel<8,gmem>",    # E = 44,000 > 39,936 LDS slots: messages in the slab
    "r510_640": "bp_generic_kernel<16,lds>",
    "r510_9000": "bp_generic_kernel<16,gmem>",  # E = 45,000
    "r324_1024": "bp_generic_kernel<32,lds>",
    "r432_2048": "bp_generic_kernel<32,lds>",
    "r432_12288": "bp_generic_kernel<32,gmem>",  # E = 49,152
    "mixA": "bp_irr_kernel<lds>",               # check degrees {2,3,5,7,8}, variable degrees 3 / 4
    "mixB": "bp_generic_kernel<32,lds>",        # check degrees {2,9,16,17,31,32}: even / odd d, padding at every width
}
_REGULAR = {"r48": (4, 8), "r58": (5, 8), "r510": (5, 10), "r324": (3, 24), "r432": (4, 32)}
_MIXED = {"mixA": (((2, 150), (3, 211), (5, 190), (7, 230), (8, 222)), 1400),
          "mixB": (((2, 40), (9, 30), (16, 25), (17, 25), (31, 12), (32, 12)), 700)}


def fallback_csr(name):
    """CSR slot form of a FALLBACK_KERNELS graph."""
    if name in _MIXED:
        classes, n = _MIXED[name]
        deg = np.concatenate([np.full(c, d) for d, c in classes])
        deg = deg[np.random.default_rng(5).permutation(deg.size)]  # degree classes interleaved
        cptr, cvar = mixed_checks(deg, n, seed=1)
        return csr_from_checks(cptr, cvar, n)
    g = fallback_regular(name)
    return csr_from_checks(np.arange(g.m + 1) * g.dc, g.check_lookup, g.n)


def fallback_regular(name):
    """The graph of a regular FALLBACK_KERNELS name r<dv><dc>_<n>, in the reference's list format."""
    kind, n = name.split("_")
    dv, dc = _REGULAR[kind]
    return regular_simple(int(n), dv, dc, seed=1)


def csr_from_checks(cptr, cvar, n):
    """CSR slot form (check_ptr, check_var, var_ptr, var_slot): each variable's slots ascending."""
    cvar = np.ascontiguousarray(cvar, np.int32)
    vslot = np.lexsort((np.arange(cvar.size), cvar)).astype(np.int32)
    vptr = np.concatenate(([0], np.cumsum(np.bincount(cvar, minlength=n)))).astype(np.int32)
    return np.ascontiguousarray(cptr, np.int32), cvar, vptr, vslot


def bp_plans(csr, calls, cus=256, env=None):
    """The soft decoders' launch plans (ldpc_debug_bp_plan, host only) of `calls` = (algo,
    early_stop, mc, want_post, iters, B) tuples on one CSR graph; env: the environment of the
    layout build (LDPC_NO_LOC_LAYOUT / LDPC_LOC_T), otherwise unset."""
    import os
    from iib_project_ldpc_codes_amd import _native
    cptr, cvar, vptr, vslot = csr
    args = np.ascontiguousarray([[B, iters, algo, es, mc, post] for algo, es, mc, post, iters, B in calls], np.int32)
    out = np.zeros((len(calls), 9), np.int64)
    names = np.zeros((len(calls), 64), np.uint8)
    saved = {k: os.environ.pop(k, None) for k in ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T")}
    os.environ.update(env or {})
    try:
        rc = _native.lib().ldpc_debug_bp_plan(cptr.ctypes.data, cvar.ctypes.data, vptr.ctypes.data, vslot.ctypes.data,
                                              vptr.size - 1, cptr.size - 1, len(calls), args.ctypes.data, cus,
                                              out.ctypes.data, names.ctypes.data)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert rc == 0, _native.last_error()
    keys = ("path", "threads", "grid", "lds", "lds_slots", "persistent", "slab", "counter", "scratch")
    plans = [dict(zip(keys, (int(x) for x in row))) for row in out]
    for p, nm in zip(plans, names):
        p["name"] = nm.tobytes().split(b"\0")[0].decode()
    return plans


BEC_DECODE, BEC_MC, BEC_ENS_MC = 0, 1, 2
BEC_KERNELS = ("Word", "DecBits", "McBits", "Peel", "None")


def bec_plans(n, m, calls, dc=6):
    """The BEC decoders' launch plans (ldpc_debug_bec_plan, host only) of `calls` = (mode, B,
    iters[, peel_cap]) tuples on a graph of n variables and m checks of degree dc."""
    from iib_project_ldpc_codes_amd import _native
    args = np.ascontiguousarray([tuple(c) + (0,) * (4 - len(c)) for c in calls], np.int32)
    out = np.zeros((len(calls), 9), np.int64)
    names = np.zeros((len(calls), 64), np.uint8)
    rc = _native.lib().ldpc_debug_bec_plan(n, m, dc, len(calls), args.ctypes.data, out.ctypes.data, names.ctypes.data)
    assert rc == 0, _native.last_error()
    keys = ("kernel", "threads", "W", "plane", "cw_per_wg", "grid", "lds", "F", "cap")
    plans = [dict(zip(keys, (int(x) for x in row))) for row in out]
    for p, nm in zip(plans, names):
        p["kernel"] = BEC_KERNELS[p["kernel"]]
        p["name"] = nm.tobytes().split(b"\0")[0].decode()
    return plans
