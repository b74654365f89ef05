"""Codes and launch plans the quasi-cyclic tests share (tests/test_qc_*.py, tests/test_gpu_qc.py)."""
import contextlib
import functools
import os

import numpy as np

from tests.layered_q_util import Q_KEYS

QC64x8, QC64x16, QC64x32, QC256x8, QC256x16, QC256x32 = range(25, 31)  # BpPath values, after bp_layer_q_kernel's
LDS_CAP = 160 * 1024 - 4096

# hand_z31: a masked 4 x 12 base, Z = 31, with shifts 0 and Z - 1 present and block-row degrees
# 1, 2, 5 and 8 (every block column used; no 4-cycle: tests/test_qc_host.py)
_X = -1
HAND_Z31 = [[_X, _X, _X, _X, _X, _X, _X, _X, _X, _X, _X, 30],
            [0, _X, _X, _X, _X, _X, _X, _X, _X, _X, 17, _X],
            [5, 0, 11, _X, _X, _X, _X, _X, 23, 30, _X, _X],
            [0, 1, 3, 7, 12, 20, 30, 9, _X, _X, _X, _X]]

# mix3x12_z67: random_base(3, 12, 67, seed=5) with zero blocks at row 1 columns 9-11 and row 2 columns 2-8
MIX3X12_MASK = [[c in cols for c in range(12)] for cols in ((), range(9, 12), range(2, 9))]
MIX3X12_Z67 = [[44, 53, 1, 54, 31, 34, 42, 19, 65, 3, 18, 25],
               [38, 27, 8, 3, 0, 9, 66, 12, 43, _X, _X, _X],
               [50, 15, _X, _X, _X, _X, _X, _X, _X, 18, 29, 17]]


@functools.lru_cache(maxsize=None)
def code(name):
    """The QCCode of a case name of tests/test_gpu_qc.py."""
    from iib_project_ldpc_codes_amd import qc
    if name.startswith("arr36_z"):
        return qc.array_code(3, 6, int(name[7:]))
    if name.startswith("rnd36_z"):
        return qc.random_base(3, 6, int(name[7:]), seed=5)
    if name == "hand_z31":
        return qc.QCCode(HAND_Z31, 31)
    if name == "dense2x12_z37":
        return qc.random_base(2, 12, 37, seed=5)
    if name == "dense2x20_z23":
        return qc.random_base(2, 20, 23, seed=5)
    # the shapes of the 16- and 32-wide codeword mode and of the 256-thread wide kernels (all full rank)
    if name == "rnd3x12_z37":  # n = 444 = 4 * 111: a multiple of 4, not of 32
        return qc.random_base(3, 12, 37, seed=5)
    if name == "rnd3x20_z61":  # n = 1,220: 305 words of P > 4 * 64
        return qc.random_base(3, 20, 61, seed=5)
    if name == "mix3x12_z67":  # n = 804; block-row degrees 12, 9 and 5 on a 16-wide kernel
        c = qc.random_base(3, 12, 67, seed=5, mask=MIX3X12_MASK)
        assert c.base.tolist() == MIX3X12_Z67, c.base.tolist()  # a change of the generator is noticed
        return c
    if name == "rnd3x20_z257":  # n = 5,140: 1,285 words of P > 4 * 256; two checks per thread, a tail of one
        return qc.random_base(3, 20, 257, seed=5)
    if name == "z1":  # the base is H itself: a 6 x 12 parity-check matrix of row degrees 4 and column degrees 2
        H = np.full((6, 12), -1)
        for c in range(12):  # column c: checks c mod 6 and (c mod 6 + 1 + c // 6) mod 6
            H[c % 6, c] = H[(c % 6 + 1 + c // 6) % 6, c] = 0
        return qc.QCCode(H, 1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def graph(name):
    return code(name).graph()


@contextlib.contextmanager
def table_kernels():
    """LDPC_NO_QC_KERNEL=1 while graphs are created: the block-row schedule on the table kernels."""
    old = os.environ.get("LDPC_NO_QC_KERNEL")
    os.environ["LDPC_NO_QC_KERNEL"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["LDPC_NO_QC_KERNEL"]
        else:
            os.environ["LDPC_NO_QC_KERNEL"] = old


def qc_plans(c, calls, cus=256, rc_only=False):
    """bp_layer_q_plan of a QCCode (ldpc_debug_qc_plan, host only) for `calls` = (algo, early_stop,
    mc, want_post, iters, B) tuples, as layered_q_util.layer_q_plans."""
    from iib_project_ldpc_codes_amd import _native
    args = np.ascontiguousarray([[B, iters, algo, es, mc, post] for algo, es, mc, post, iters, B in calls],
                                np.int32).reshape(len(calls), 6)
    out = np.zeros((len(calls), 9), np.int64)
    names = np.zeros((len(calls), 64), np.uint8)
    rc = _native.lib().ldpc_debug_qc_plan(c.mb, c.nb, c.Z, c.base.ctypes.data, len(calls), args.ctypes.data, cus,
                                          out.ctypes.data, names.ctypes.data)
    if rc_only:
        return rc
    assert rc == 0, _native.last_error()
    plans = [dict(zip(Q_KEYS, (int(x) for x in row))) for row in out]
    for p, nm in zip(plans, names):
        p["name"] = nm.tobytes().split(b"\0")[0].decode()
    return plans


def kernel_name(c):
    """The display name bp_layer_q_plan must give a quasi-cyclic code."""
    d = int((c.base >= 0).sum(axis=1).max())
    return "bp_qc_q_kernel<%d,%d>" % (64 if c.Z <= 64 else 256, 8 if d <= 8 else 16 if d <= 16 else 32)
