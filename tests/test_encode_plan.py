"""encode_plan (csrc/encode_plan.cpp, read through ldpc_debug_encode_plan without a device): literal
rows at the boundaries of the tile ladder, worked out by hand from the rule.

The rule: a workgroup encodes 32 W codewords from K information planes of 4 W bytes each in LDS; W is
the widest of 4, 2, 1 with 4 K W <= 160 KiB - 4 KiB = 159,744, so W = 4 up to K = 9,984, W = 2 up to
K = 19,968, W = 1 up to K = 39,936 and no plan beyond.  1,024 threads when the planes take more than
half a CU's LDS (81,920 bytes), else 256.  grid = ceil(B / 32 W); the parity planes are one uint32 per
(plane word, parity row): scratch = 4 rank grid W; the write pass has one thread per 4 variables of a
codeword in workgroups of 256.
"""
from iib_project_ldpc_codes_amd import _native
from tests import encode_util as eu

CAP = 160 * 1024 - 4096
NONE = {"threads": 0, "W": 0, "cw_per_wg": 0, "grid": 0, "lds": 0, "cap": 0, "pwords": 0, "scratch": 0,
        "write_grid": 0, "name": "none"}


def _row(threads, W, grid, lds, rank, write_grid):
    return {"threads": threads, "W": W, "cw_per_wg": 32 * W, "grid": grid, "lds": lds, "cap": CAP, "pwords": grid * W,
            "scratch": 4 * rank * grid * W, "write_grid": write_grid, "name": "encode_parity_kernel<%d>" % W}


def test_ladder_boundaries():
    calls = [(1000, 500, 500, 257),        # 8,000 bytes; 257 codewords: 3 tiles of 128; 250 * 257 threads
             (10000, 5000, 5000, 65536),   # the headline shape: 80,000 bytes, two workgroups per CU
             (10240, 5120, 5120, 128),     # 81,920 bytes: exactly half the LDS, still 256 threads
             (10242, 5121, 5121, 128),     # 81,936 bytes: past half, 1,024 threads
             (19968, 9984, 9984, 129),     # the last K at W = 4: 159,744 bytes
             (19970, 9985, 9985, 129),     # W = 2: 79,880 bytes, 3 tiles of 64
             (39936, 19968, 19968, 64),    # the last K at W = 2
             (39938, 19969, 19969, 65),    # W = 1: 79,876 bytes, 3 tiles of 32
             (64800, 32400, 32400, 1),     # the DVB-S2 length: W = 1, 129,600 bytes
             (79872, 39936, 39936, 33),    # the last K at W = 1
             (40, 0, 40, 33)]              # K = 0: no planes at all
    rc, rows = eu.encode_plans(calls)
    assert rc == 0
    assert rows == [_row(256, 4, 3, 8000, 500, 251),
                    _row(256, 4, 512, 80000, 5000, 640000),
                    _row(256, 4, 1, 81920, 5120, 1280),
                    _row(1024, 4, 1, 81936, 5121, 1281),
                    _row(1024, 4, 2, 159744, 9984, 2516),
                    _row(256, 2, 3, 79880, 9985, 2517),
                    _row(1024, 2, 1, 159744, 19968, 2496),
                    _row(256, 1, 3, 79876, 19969, 2536),
                    _row(1024, 1, 1, 129600, 32400, 64),
                    _row(1024, 1, 2, 159744, 39936, 2574),
                    _row(256, 4, 1, 0, 40, 2)]


def test_no_plan_is_unsupported():
    # K = 39,937 fits nothing at W = 1; the fitting call beside it is still answered
    rc, rows = eu.encode_plans([(79874, 39937, 39937, 32), (1000, 500, 500, 32)])
    assert rc == _native.LDPC_EUNSUP and "fit LDS" in _native.last_error()
    assert rows[0] == NONE
    assert rows[1] == _row(256, 4, 1, 8000, 500, 32)


def test_empty_batch_and_bad_arguments():
    rc, rows = eu.encode_plans([(1000, 500, 500, 0)])
    assert rc == 0 and rows[0]["grid"] == 0 and rows[0]["scratch"] == 0 and rows[0]["write_grid"] == 0
    for bad in [(1000, 500, 499, 1), (0, 0, 0, 1), (1000, 500, 500, -1), (10, -1, 11, 1)]:
        assert eu.encode_plans([bad])[0] == _native.LDPC_EINVAL
