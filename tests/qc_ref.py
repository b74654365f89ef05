"""An independent numpy expansion of a quasi-cyclic base matrix: H as a sum of shifted identities.

Convention (include/ldpc_mi355x.h, ldpc_graph_create_qc): check r Z + i holds variable
c Z + (i + s_rc) mod Z for every non-zero cell of block row r, in ascending block-column order (the
slot order); a variable's checks are in ascending check id.
"""
import numpy as np


def dense(base, Z):
    """H uint8 [mb Z, nb Z]: block (r, c) is the identity with its columns rolled right by s_rc."""
    base = np.asarray(base)
    mb, nb = base.shape
    H = np.zeros((mb * Z, nb * Z), np.uint8)
    eye = np.eye(Z, dtype=np.uint8)
    for r in range(mb):
        for c in range(nb):
            if base[r, c] >= 0:
                H[r * Z:(r + 1) * Z, c * Z:(c + 1) * Z] += np.roll(eye, int(base[r, c]), axis=1)
    return H


def csr(base, Z):
    """(check_ptr, check_var, var_ptr, var_slot) read off the dense H: a check's variables
    ascending (= ascending block column: one per block), a variable's slots ascending with the check."""
    H = dense(base, Z)
    assert H.max() == 1
    m, n = H.shape
    rows = [np.nonzero(H[c])[0] for c in range(m)]
    cptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int32)
    cvar = np.concatenate(rows).astype(np.int32)
    slot_of = {}
    for c in range(m):
        for j, v in enumerate(rows[c]):
            slot_of[(c, int(v))] = int(cptr[c]) + j
    vptr, vslot = [0], []
    for v in range(n):
        for c in np.nonzero(H[:, v])[0]:
            vslot.append(slot_of[(int(c), v)])
        vptr.append(len(vslot))
    return cptr, cvar, np.asarray(vptr, np.int32), np.asarray(vslot, np.int32)
