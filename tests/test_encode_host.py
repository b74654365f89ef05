"""The systematic encoder description (csrc/encode_host.cpp, read through ldpc_debug_encoder_build
without a device) against tests/encode_ref.py, an independent numpy elimination: the positions
partition the variables, the rank is the reference's, the parity columns are independent, and A is
the reference's solution on every unit vector -- which pins A without pinning the pivot rule.
"""
import numpy as np
import pytest

from tests import encode_ref, encode_util as eu


@pytest.mark.parametrize("name", eu.NAMES)
def test_description_against_reference(name):
    H = eu.H(name)
    m, n = H.shape
    rank, info, par, A = eu.description(name)
    K = n - rank
    assert rank == encode_ref.rank(H)
    assert info.size == K and par.size == rank
    assert sorted(np.concatenate([info, par]).tolist()) == list(range(n))  # a partition of 0..n-1
    assert (np.diff(info) > 0).all()  # ascending
    assert encode_ref.rank(H[:, par]) == rank  # H[:, par] has independent columns: invertible on its row space
    bits, pad = encode_ref.unpack_rows(A, K)
    assert A.shape == (rank, (K + 31) // 32) and not pad.any()  # the padding bits are zero
    # unit vectors: column j of A is the parity part of the codeword with u = e_j
    x = encode_ref.solve(H, info, par, np.eye(K, dtype=np.uint8))
    np.testing.assert_array_equal(bits, x[:, par].T)
    assert not (H.astype(np.int64) @ x.T.astype(np.int64) & 1).any()


def test_shapes_the_graphs_are_there_for():
    rank = {name: eu.description(name)[0] for name in eu.NAMES}
    n = {name: eu.graph(name)[2] for name in eu.NAMES}
    assert rank["r48_64"] < 32  # rank-deficient: K > k = 32
    assert n["square"] - rank["square"] == 0  # K = 0: the code is {0}
    assert n["r36_96"] - rank["r36_96"] >= 48 and (n["r36_96"] - rank["r36_96"]) % 32  # a partial word of A
    assert n["r36_1000"] - rank["r36_1000"] == 500  # rank 500: K = k
    assert 96 in eu.description("lonely")[1]  # the variable in no check is an information position
    # the doubled slot cancels: H of `twice` differs from r36_96's in check 0 alone
    d = eu.H("twice") ^ eu.H("r36_96")
    assert d[0].sum() == 2 and not d[1:].any()


@pytest.mark.parametrize("name", ["r36_96", "mixB", "r48_64"])
def test_two_builds_agree(name):
    a, b = eu.description(name), eu.description(name)
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)


def test_parity_sits_at_the_high_end():
    """The rule scans columns downward: on a graph whose last rank columns are independent they are
    the parity positions, in falling order."""
    rank, info, par, _ = eu.description("square")
    assert par.tolist() == list(range(39, -1, -1)) and info.size == 0
    rank, info, par, _ = eu.description("r36_1000")
    assert (np.diff(par) < 0).all() and par[0] == 999


def test_bad_arguments():
    from iib_project_ldpc_codes_amd import _native
    import ctypes as ct
    L = _native.lib()
    cptr, cvar, n = eu.graph("r36_12")
    rank = ct.c_int32(0)
    assert L.ldpc_debug_encoder_build(cptr.ctypes.data, cvar.ctypes.data, n, cptr.size - 1, None, None, None,
                                      None) == _native.LDPC_EINVAL
    bad = cvar.copy()
    bad[3] = n
    assert L.ldpc_debug_encoder_build(cptr.ctypes.data, bad.ctypes.data, n, cptr.size - 1, ct.addressof(rank), None,
                                      None, None) == _native.LDPC_EINVAL
    assert L.ldpc_encode_rule().decode().startswith("gauss-jordan/columns-descending")
