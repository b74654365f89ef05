"""An independent numpy GF(2) elimination for the encoder tests: H of a CSR check side, rank(H), and
solve, the unique x with x[info] = u and H x = 0.

Uniqueness: the parity columns of a valid encoder description are independent (H[:, par] has full
column rank = rank(H)), so the parity bits are determined by the information bits whatever pivot rule
found the positions -- the tests pin the encoder without pinning its rule.  Plain dense uint8
arithmetic, columns scanned upward: nothing is shared with csrc/encode_host.cpp.
"""
import numpy as np


def parity_matrix(check_ptr, check_var, n):
    """Dense H uint8 [m, n]: entry (c, v) = parity of the number of slots of check c that hold v."""
    cptr = np.asarray(check_ptr, np.int64)
    m = cptr.size - 1
    H = np.zeros((m, n), np.uint8)
    chk = np.repeat(np.arange(m), np.diff(cptr))
    np.add.at(H, (chk, np.asarray(check_var, np.int64)), 1)
    return H & 1


def _eliminate(M, ncols):
    """Row-reduce a copy of M (uint8) on its first ncols columns.  Returns (reduced, pivot columns)."""
    M = M.copy()
    rows = M.shape[0]
    r, piv = 0, []
    for c in range(ncols):
        if r == rows:
            break
        hit = np.nonzero(M[r:, c])[0]
        if not hit.size:
            continue
        p = r + hit[0]
        if p != r:
            M[[r, p]] = M[[p, r]]
        others = np.nonzero(M[:, c])[0]
        others = others[others != r]
        M[others] ^= M[r]
        piv.append(c)
        r += 1
    return M, piv


def rank(H):
    return len(_eliminate(np.asarray(H, np.uint8) & 1, H.shape[1])[1])


def solve(H, info_pos, par_pos, U):
    """Codewords x uint8 [B, n] with x[:, info_pos] = U and H x = 0, for U uint8 [B, K].  Asserts that
    the parity columns are independent and that the system is consistent (so x is unique)."""
    H = np.asarray(H, np.uint8) & 1
    n = H.shape[1]
    info_pos, par_pos = np.asarray(info_pos, np.int64), np.asarray(par_pos, np.int64)
    U = np.atleast_2d(np.asarray(U, np.uint8)) & 1
    B, r = U.shape[0], par_pos.size
    rhs = (H[:, info_pos].astype(np.int64) @ U.T.astype(np.int64) & 1).astype(np.uint8)  # [m, B]
    red, piv = _eliminate(np.concatenate([H[:, par_pos], rhs], axis=1), r)
    assert piv == list(range(r)), "the parity columns are dependent"
    assert not red[r:, r:].any(), "no codeword has these information bits"
    x = np.zeros((B, n), np.uint8)
    x[:, info_pos] = U
    x[:, par_pos] = red[:r, r:].T  # reduced to the identity on the parity columns
    return x


def unpack_rows(A_words, K):
    """Packed A uint32 [rank, ceil(K / 32)] -> bits uint8 [rank, K] and the padding bits [rank, pad]."""
    A = np.asarray(A_words, np.uint32)
    bits = (A[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :] & 1).astype(np.uint8).reshape(A.shape[0], -1)
    return bits[:, :K], bits[:, K:]
