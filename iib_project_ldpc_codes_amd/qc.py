"""Quasi-cyclic codes: H is an mb x nb array of Z x Z circulant permutations or zero blocks.

``QCCode(base, Z)`` describes one: ``base`` int [mb][nb], -1 for a zero block, otherwise a shift
0 <= s < Z.  Expansion convention (include/ldpc_mi355x.h, ldpc_graph_create_qc): check r Z + i
holds variable c Z + (i + s_rc) mod Z for every non-zero cell of block row r, in ascending
block-column order (the slot order); a variable's checks are in ascending check id.

``QCCode.graph()`` is a TannerGraph every decoder, the encoder and the Monte-Carlo engine take as
any other.  Its layers are its block rows (rule "qc/block-row/v1"), not a colouring, and the
fixed-point layered min-sum runs bp_qc_q_kernel on it, which forms a check's variables from the
block row's shifts instead of reading index tables.

Constructors: ``array_code`` (shift r c mod Z, Z prime), ``random_base`` (numpy PCG64 shifts, redrawn
while they close a 4-cycle), ``QCCode.from_text`` (a standard's table brought by the user).
"""
import ctypes as ct

import numpy as np

from . import _native
from .graph import TannerGraph

LAYER_RULE = "qc/block-row/v1"
MAX_ROW_DEGREE = 32


class QCCode:
    def __init__(self, base, Z):
        base = np.array(base, dtype=np.int64, ndmin=2)
        if base.ndim != 2 or base.size == 0:
            raise ValueError("QCCode: base must be a non-empty [mb][nb] array")
        if isinstance(Z, bool) or int(Z) != Z or int(Z) < 1:
            raise ValueError("QCCode: need an integer Z >= 1")
        Z = int(Z)
        if np.any(base < -1) or np.any(base >= Z):
            raise ValueError("QCCode: an entry is -1 (zero block) or a shift in [0, Z)")
        nz = base >= 0
        if not nz.any(axis=1).all():
            raise ValueError("QCCode: an all-zero block row")
        if not nz.any(axis=0).all():
            raise ValueError("QCCode: an all-zero block column")
        if nz.sum(axis=1).max() > MAX_ROW_DEGREE:
            raise ValueError(f"QCCode: a block row has more than {MAX_ROW_DEGREE} non-zero blocks")
        self.base = np.ascontiguousarray(base, np.int32)
        self.Z = Z
        self.mb, self.nb = self.base.shape

    @property
    def n(self):
        return self.nb * self.Z

    @property
    def m(self):
        return self.mb * self.Z

    # ------------------------------------------------------------------- text
    @classmethod
    def from_text(cls, path, Z):
        """Whitespace-separated rows of integers, -1 for a zero block; blank lines and lines
        starting with '#' are skipped.  Z is the caller's."""
        rows = []
        with open(path) as f:
            for line in f:
                line = line.strip()
                if line and not line.startswith("#"):
                    rows.append([int(x) for x in line.split()])
        if not rows or any(len(r) != len(rows[0]) for r in rows):
            raise ValueError(f"{path}: rows of different lengths (or none)")
        return cls(rows, Z)

    def to_text(self, path):
        with open(path, "w") as f:
            for row in self.base:
                f.write(" ".join(str(int(x)) for x in row) + "\n")

    # ------------------------------------------------------------------ graph
    def expand(self):
        """(check_ptr, check_var, var_ptr, var_slot, layer) of the expansion (ldpc_debug_qc_expand,
        host only)."""
        E = int((self.base >= 0).sum()) * self.Z
        cptr, cvar = np.zeros(self.m + 1, np.int32), np.zeros(E, np.int32)
        vptr, vslot = np.zeros(self.n + 1, np.int32), np.zeros(E, np.int32)
        layer = np.zeros(self.m, np.int32)
        rc = _native.lib().ldpc_debug_qc_expand(self.mb, self.nb, self.Z, self.base.ctypes.data, cptr.ctypes.data,
                                                cvar.ctypes.data, vptr.ctypes.data, vslot.ctypes.data,
                                                layer.ctypes.data)
        _native.check(rc, "ldpc_debug_qc_expand")
        return cptr, cvar, vptr, vslot, layer

    def graph(self):
        return QCGraph(self)

    def rate_match(self, punctured_cols=(), shortened_cols=(), count="codeword"):
        """A ratematch.RateMatch of whole block columns: column c stands for its Z variables c Z ..
        c Z + Z - 1 (5G NR never sends its first two block columns)."""
        from .ratematch import RateMatch

        def expand(what, cols):
            cols = np.asarray(cols, dtype=np.int64).ravel()
            if cols.size and (cols.min() < 0 or cols.max() >= self.nb):
                raise ValueError(f"QCCode.rate_match: a {what} block column outside [0, {self.nb})")
            return (cols[:, None] * self.Z + np.arange(self.Z)[None, :]).ravel()
        return RateMatch(self.n, expand("punctured", punctured_cols), expand("shortened", shortened_cols), count)


class QCGraph(TannerGraph):
    """The expansion of a QCCode: a CSR TannerGraph whose device handle is made by
    ldpc_graph_create_qc and whose layers are the block rows."""
    layer_rule = LAYER_RULE

    def __init__(self, code):
        self.code = code
        self.csr = tuple(code.expand()[:4])
        self.m, self.n = code.m, code.n
        self.k = self.n - self.m
        self.dv = self.dc = 0
        self.variable_lookup = self.check_lookup = None
        self._handles = {}

    def handle(self):
        dev = 0
        try:
            import torch
            if torch.cuda.is_available():
                dev = torch.cuda.current_device()
        except Exception:
            pass
        h = self._handles.get(dev)
        if h is not None:
            return h
        out = ct.c_void_p()
        c = self.code
        rc = _native.lib().ldpc_graph_create_qc(c.mb, c.nb, c.Z, c.base.ctypes.data, ct.byref(out))
        _native.check(rc, "ldpc_graph_create_qc")
        self._handles[dev] = out
        return out

    def layer_schedule(self):
        """The block row of every check: check // Z."""
        return (np.arange(self.m, dtype=np.int32) // self.code.Z).astype(np.int32)


def _is_prime(z):
    return z >= 2 and all(z % p for p in range(2, int(z ** 0.5) + 1))


def array_code(dv, dc, Z):
    """The (dv, dc) array code: shift (r c) mod Z in cell (r, c) of a dv x dc base, Z prime and
    >= max(dv, dc).  No 4-cycles: (r1 - r2)(c1 - c2) is not 0 mod Z.  Z = 1667 is the (3,6)
    n = 10,002 twin of the (3,6) n = 10,000 headline code."""
    if dv < 1 or dc < 1 or not _is_prime(Z) or Z < max(dv, dc):
        raise ValueError("array_code: need dv, dc >= 1 and a prime Z >= max(dv, dc)")
    r, c = np.arange(dv)[:, None], np.arange(dc)[None, :]
    return QCCode((r * c) % Z, Z)


MAX_REDRAWS = 1000  # of one cell, before random_base gives up


def random_base(mb, nb, Z, seed, mask=None):
    """Shifts drawn by numpy PCG64(seed), cell by cell in row-major order; a cell is redrawn while
    it closes a 4-cycle with the cells before it, i.e. while s[r1][c1] - s[r1][c2] + s[r2][c2] -
    s[r2][c1] = 0 (mod Z) over non-zero cells.  mask [mb][nb]: true marks a zero block.
    RuntimeError after MAX_REDRAWS redraws of one cell."""
    rng = np.random.Generator(np.random.PCG64(seed))
    zero = np.zeros((mb, nb), bool) if mask is None else np.asarray(mask, bool)
    if zero.shape != (mb, nb):
        raise ValueError("random_base: mask must be [mb][nb]")
    s = np.full((mb, nb), -1, np.int64)

    def closes(r, c):
        for r2 in range(r + 1):
            for c2 in range(nb):
                if r2 == r or c2 == c or min(s[r2, c2], s[r2, c], s[r, c2]) < 0:
                    continue
                if (s[r, c] - s[r, c2] + s[r2, c2] - s[r2, c]) % Z == 0:
                    return True
        return False

    for r in range(mb):
        for c in range(nb):
            if zero[r, c]:
                continue
            for _ in range(MAX_REDRAWS + 1):
                s[r, c] = int(rng.integers(Z))
                if not closes(r, c):
                    break
            else:
                raise RuntimeError(f"random_base: cell ({r}, {c}) closes a 4-cycle at every one of "
                                   f"{MAX_REDRAWS + 1} draws (Z = {Z} too small for this base)")
    return QCCode(s, Z)
