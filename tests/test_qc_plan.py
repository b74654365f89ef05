"""bp_layer_q_plan on quasi-cyclic codes (ldpc_debug_qc_plan, host only): literal rows.  Columns:
path, threads, grid, LDS bytes, workgroups per CU, persistent, slab, counter, scratch."""
import numpy as np
import pytest

from iib_project_ldpc_codes_amd import _native, qc
from tests.layered_q_util import LQ8
from tests.qc_util import (LDS_CAP, QC64x8, QC64x16, QC64x32, QC256x8, QC256x16, QC256x32, code, kernel_name, qc_plans,
                           table_kernels)

DECODE, MC = (1, 0, 0, 1, 20, 24), (1, 1, 1, 0, 20, 128)  # algo, early_stop, mc, want_post, iters, B


def _row(p):
    return (p["name"], p["path"], p["threads"], p["grid"], p["lds"], p["wg_per_cu"], p["scratch"])


def _wide(d, Z):
    """One block row of degree d (shifts 0: a single row closes no cycle) over d block columns."""
    return qc.QCCode(np.zeros((1, d), int), Z)


def test_threads_on_both_sides_of_z_64():
    # (3,6): n = 6 Z, m = 3 Z, 4-byte records: LDS = pad4(6 Z) + 12 Z; the curve of 20 iterations: 96 bytes
    assert [_row(p) for p in qc_plans(code("rnd36_z64"), [DECODE, MC])] == [
        ("bp_qc_q_kernel<64,8>", QC64x8, 64, 24, 384 + 768, 32, 0),
        ("bp_qc_q_kernel<64,8>", QC64x8, 64, 128, 96 + 384 + 768, 32, 0)]
    assert [_row(p) for p in qc_plans(code("rnd36_z65"), [DECODE, MC])] == [
        ("bp_qc_q_kernel<256,8>", QC256x8, 256, 24, 392 + 780, 8, 0),
        ("bp_qc_q_kernel<256,8>", QC256x8, 256, 128, 96 + 392 + 780, 8, 0)]
    assert _row(qc_plans(code("arr36_z7"), [DECODE])[0]) == ("bp_qc_q_kernel<64,8>", QC64x8, 64, 24, 44 + 84, 32, 0)
    assert _row(qc_plans(code("z1"), [DECODE])[0]) == ("bp_qc_q_kernel<64,8>", QC64x8, 64, 24, 12 + 24, 32, 0)


def test_width_on_both_sides_of_degree_8_and_16():
    # one block row of degree d, Z = 5 and Z = 70: n = d Z, m = Z
    want = {8: (8, QC64x8, QC256x8, 4), 9: (16, QC64x16, QC256x16, 4), 16: (16, QC64x16, QC256x16, 4),
            17: (32, QC64x32, QC256x32, 8), 32: (32, QC64x32, QC256x32, 8)}
    for d, (w, p64, p256, rec) in want.items():
        for Z, T, path, per_cu in ((5, 64, p64, 32), (70, 256, p256, 8)):
            c = _wide(d, Z)
            lds = (d * Z + 3) // 4 * 4 + rec * Z
            assert _row(qc_plans(c, [DECODE])[0]) == ("bp_qc_q_kernel<%d,%d>" % (T, w), path, T, 24, lds, per_cu, 0)
            assert kernel_name(c) == "bp_qc_q_kernel<%d,%d>" % (T, w)
    assert _row(qc_plans(code("dense2x12_z37"), [DECODE])[0]) == ("bp_qc_q_kernel<64,16>", QC64x16, 64, 24,
                                                                   444 + 4 * 74, 32, 0)
    assert _row(qc_plans(code("dense2x20_z23"), [DECODE])[0]) == ("bp_qc_q_kernel<64,32>", QC64x32, 64, 24,
                                                                   460 + 8 * 46, 32, 0)
    assert _row(qc_plans(code("hand_z31"), [DECODE])[0]) == ("bp_qc_q_kernel<64,8>", QC64x8, 64, 24, 372 + 4 * 124,
                                                              32, 0)


def test_the_cap_and_the_headline_shape():
    # the (3,6) array codes: LDS = pad4(6 Z) + 12 Z <= 160 KiB - 4 KiB up to Z = 8,874 (prime: 8,867 and 8,887)
    assert LDS_CAP == 159744
    last, first = qc.array_code(3, 6, 8867), qc.array_code(3, 6, 8887)
    assert _row(qc_plans(last, [DECODE])[0]) == ("bp_qc_q_kernel<256,8>", QC256x8, 256, 24, 53204 + 106404, 1, 0)
    assert 53204 + 106404 <= LDS_CAP < 53324 + 106644
    assert _row(qc_plans(first, [DECODE])[0]) == ("none", 9, 0, 0, 0, 0, 0)
    # the curve counts: 40,000 iterations leave no room
    assert qc_plans(code("arr36_z67"), [(1, 1, 1, 0, 40000, 128)])[0]["name"] == "none"
    # the (3,6) Z = 1667 twin of the headline code: 10,004 + 20,004 bytes, five workgroups per CU
    head = qc.array_code(3, 6, 1667)
    assert _row(qc_plans(head, [(1, 1, 0, 0, 50, 16384)])[0]) == ("bp_qc_q_kernel<256,8>", QC256x8, 256, 16384, 30008,
                                                                   5, 0)
    # the same graph kept on the table kernel
    with table_kernels():
        assert _row(qc_plans(head, [(1, 1, 0, 0, 50, 16384)])[0]) == ("bp_layer_q_kernel<8>", LQ8, 256, 16384, 30008,
                                                                       5, 0)
    assert qc_plans(head, [(1, 1, 0, 0, 50, 16384)])[0]["name"] == "bp_qc_q_kernel<256,8>"


def test_bad_arguments():
    c = code("arr36_z7")
    b = c.base
    L = _native.lib()
    out, names, calls = np.zeros(9, np.int64), np.zeros(64, np.uint8), np.asarray([24, 20, 1, 0, 0, 1], np.int32)
    assert L.ldpc_debug_qc_plan(3, 6, 7, b.ctypes.data, 1, calls.ctypes.data, 256, out.ctypes.data,
                                names.ctypes.data) == 0
    assert L.ldpc_debug_qc_plan(3, 6, 5, b.ctypes.data, 1, calls.ctypes.data, 256, out.ctypes.data,
                                names.ctypes.data) == _native.LDPC_EINVAL  # a shift of 5 and of 6 at Z = 5
    assert L.ldpc_debug_qc_plan(3, 6, 7, b.ctypes.data, 1, None, 256, out.ctypes.data,
                                names.ctypes.data) == _native.LDPC_EINVAL
    assert L.ldpc_debug_qc_plan(3, 6, 7, None, 1, calls.ctypes.data, 256, out.ctypes.data,
                                names.ctypes.data) == _native.LDPC_EINVAL
