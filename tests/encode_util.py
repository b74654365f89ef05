"""The graphs of the encoder tests (tests/test_encode_host.py, tests/test_encode_host_san.py,
tests/test_gpu_encode.py) and the library's description of them.

name -> (check_ptr, check_var, n):
  r36_12, r36_96, r36_1000   (3,6)-regular; K = n / 2 unless rows depend (96: one partial word of A,
                             1000: the graph of the Monte-Carlo tests, K = 500, a tail word)
  r48_64                     (4,8)-regular: even dv, the rows sum to zero, rank < m and K > k
  mixA, mixB                 tests.graph_util.mixed_checks irregular graphs (n = 1,400 / 700)
  twice                      r36_96 with check 0 holding its first variable twice (the pair cancels)
  lonely                     r36_96 on 97 variables: variable 96 is in no check (an information position)
  square                     40 checks on 40 variables, H lower bidiagonal: full rank, K = 0
"""
import functools

import numpy as np

from tests import graph_util

NAMES = ("r36_12", "r36_96", "r36_1000", "r48_64", "mixA", "mixB", "twice", "lonely", "square")
GPU_NAMES = tuple(n for n in NAMES if n != "mixA")  # n <= 1,000
# wide_<K>: the smallest K whose information planes leave the tile of 4 plane words, and of 2 (4 K W bytes
# past 160 - 4 KiB): the encoder's tiles of 2 and of 1
TILE_NAMES = (("wide_9985", 2), ("wide_19969", 1))


@functools.lru_cache(maxsize=None)
def graph(name):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    if name in ("r36_96", "r36_1000"):
        g = TannerGraph.random_regular(int(name.split("_")[1]), 3, 6, seed=1)
    elif name == "r36_12":
        g = graph_util.regular_simple(12, 3, 6, seed=1)
    elif name == "r48_64":
        g = graph_util.regular_simple(64, 4, 8, seed=1)
    elif name in ("mixA", "mixB"):
        csr = graph_util.fallback_csr(name)
        return _frozen(csr[0], csr[1], csr[2].size - 1)
    elif name == "twice":
        cptr, cvar, _ = graph("r36_96")
        cvar = cvar.copy()
        cvar[1] = cvar[0]
        return _frozen(cptr, cvar, 96)
    elif name == "lonely":
        cptr, cvar, _ = graph("r36_96")
        return _frozen(cptr, cvar, 97)
    elif name.startswith("wide_"):
        # 16 disjoint checks over K + 16 variables (variable v in check v mod 16): rank 16, K information bits
        n = int(name.split("_")[1]) + 16
        cvar = np.concatenate([np.arange(c, n, 16) for c in range(16)])
        cptr = np.concatenate([[0], np.cumsum([len(range(c, n, 16)) for c in range(16)])])
        return _frozen(cptr, cvar, n)
    elif name == "square":
        cvar = np.concatenate([[0]] + [[c, c - 1] for c in range(1, 40)])
        cptr = np.concatenate([[0, 1], 1 + 2 * np.arange(1, 40)])
        return _frozen(cptr, cvar, 40)
    else:
        raise KeyError(name)
    return _frozen(np.arange(g.m + 1) * g.dc, g.check_lookup, g.n)


def _frozen(cptr, cvar, n):
    out = np.ascontiguousarray(cptr, np.int32), np.ascontiguousarray(cvar, np.int32)
    for a in out:
        a.setflags(write=False)
    return out + (int(n),)


def tanner(name):
    """A fresh TannerGraph (CSR form) of the named graph."""
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    cptr, cvar, n = graph(name)
    return TannerGraph.from_csr(*graph_util.csr_from_checks(cptr, cvar, n))


@functools.lru_cache(maxsize=None)
def H(name):
    from tests import encode_ref
    cptr, cvar, n = graph(name)
    h = encode_ref.parity_matrix(cptr, cvar, n)
    h.setflags(write=False)
    return h


def description(name):
    """(rank, info_pos, par_pos, A_words) of ldpc_debug_encoder_build (host only)."""
    from iib_project_ldpc_codes_amd import encoder
    cptr, cvar, n = graph(name)
    return encoder.host_description(cptr, cvar, n)


def encode_plans(calls):
    """(rc, rows) of ldpc_debug_encode_plan for calls = (n, K, rank, B) tuples."""
    from iib_project_ldpc_codes_amd import _native
    args = np.ascontiguousarray(calls, np.int32).reshape(-1, 4)
    out = np.zeros((len(args), 9), np.int64)
    names = np.zeros((len(args), 64), np.uint8)
    rc = _native.lib().ldpc_debug_encode_plan(len(args), args.ctypes.data, out.ctypes.data, names.ctypes.data)
    keys = ("threads", "W", "cw_per_wg", "grid", "lds", "cap", "pwords", "scratch", "write_grid")
    rows = [dict(zip(keys, (int(x) for x in row))) for row in out]
    for p, nm in zip(rows, names):
        p["name"] = nm.tobytes().split(b"\0")[0].decode()
    return rc, rows
