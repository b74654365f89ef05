"""Launch plans and parameter sets the fixed-point layered min-sum tests share."""
import numpy as np

from tests.layered_util import KEYS

Q_KEYS = tuple("wg_per_cu" if k == "lds_slots" else k for k in KEYS)  # column 4 of ldpc_debug_layer_q_plan
LQ8, LQ16, LQ32 = 22, 23, 24  # BpPath values, after bp_layer_kernel's


def layer_q_plans(csr, calls, cus=256, rc_only=False):
    """bp_layer_q_plan (ldpc_debug_layer_q_plan, host only) of `calls` = (algo, early_stop, mc,
    want_post, iters, B) tuples on one CSR graph, as layered_util.layer_plans."""
    from iib_project_ldpc_codes_amd import _native
    cptr, cvar, vptr, vslot = [np.ascontiguousarray(a, np.int32) for a in csr]
    args = np.ascontiguousarray([[B, iters, algo, es, mc, post] for algo, es, mc, post, iters, B in calls],
                                np.int32).reshape(len(calls), 6)
    out = np.zeros((len(calls), 9), np.int64)
    names = np.zeros((len(calls), 64), np.uint8)
    rc = _native.lib().ldpc_debug_layer_q_plan(cptr.ctypes.data, cvar.ctypes.data, vptr.ctypes.data,
                                               vslot.ctypes.data, vptr.size - 1, cptr.size - 1, len(calls),
                                               args.ctypes.data, cus, out.ctypes.data, names.ctypes.data)
    if rc_only:
        return rc
    assert rc == 0, _native.last_error()
    plans = [dict(zip(Q_KEYS, (int(x) for x in row))) for row in out]
    for p, nm in zip(plans, names):
        p["name"] = nm.tobytes().split(b"\0")[0].decode()
    return plans


def kernel_name(csr):
    """The display name bp_layer_q_plan must give a graph: width by the largest check degree."""
    d = int(np.diff(csr[0]).max())
    return "bp_layer_q_kernel<%d>" % (8 if d <= 8 else 16 if d <= 16 else 32)


def lds_bytes(csr, iters=0, mc=False):
    """curve + pad4(n) + rec m, rec = 4 bytes up to check degree 16, else 8."""
    n, m, d = csr[2].size - 1, csr[0].size - 1, int(np.diff(csr[0]).max())
    return ((4 * (iters + 1) + 15) // 16 * 16 if mc else 0) + (n + 3) // 4 * 4 + (4 if d <= 16 else 8) * m
