"""The row I/O rule of bp_loc_kernel's fixed-count decodes, from the host plan alone
(ldpc_debug_bp_plan_io, no device needed): wide_io exactly when llr and post are 16-byte aligned
and hard 4-byte aligned (a null post or hard counts as aligned), never under LDPC_NO_WIDE_IO, for
an early-stop or Monte-Carlo call, or on another kernel; the message LDS keeps four spare words
behind the n staged values (the unguarded accesses past a row's end land there); and the first
nine fields are ldpc_debug_bp_plan's."""
import contextlib
import functools
import itertools
import os

import numpy as np
import pytest

from tests.graph_util import bp_plans

BASE = 0x7F0000000000  # a 4 KiB aligned address; nothing is read through it
SIZES = [4100, 10000, 1000]


@functools.lru_cache(maxsize=None)
def _csr(n):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    return tuple(np.ascontiguousarray(a, np.int32) for a in TannerGraph.random_regular(n, 3, 6, seed=21).to_csr())


@contextlib.contextmanager
def _layout_env(env):
    keys = ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T", "LDPC_NO_LOC_CHAIN")
    saved = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(env or {})
    try:
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def _plans(n, calls, env=None):
    """calls: (B, iters, algo, early_stop, mc, llr, post, hard, narrow) -> dicts with ldpc_debug_bp_plan's keys + wide_io, msg_words"""
    from iib_project_ldpc_codes_amd import _native
    csr = _csr(n)
    args = np.ascontiguousarray(calls, np.int64)
    out, names = np.zeros((len(calls), 11), np.int64), np.zeros((len(calls), 64), np.uint8)
    with _layout_env(env):
        rc = _native.lib().ldpc_debug_bp_plan_io(*(a.ctypes.data for a in csr), n, csr[0].size - 1, len(calls),
                                                 args.ctypes.data, 256, out.ctypes.data, names.ctypes.data)
    assert rc == 0, _native.last_error()
    keys = ("path", "threads", "grid", "lds", "lds_slots", "persistent", "slab", "counter", "scratch", "wide_io", "msg_words")
    plans = [dict(zip(keys, (int(x) for x in row))) for row in out]
    for p, nm in zip(plans, names):
        p["name"] = nm.tobytes().split(b"\0")[0].decode()
    return plans


@pytest.mark.parametrize("env", [None, {"LDPC_NO_LOC_CHAIN": "1"}], ids=["chain", "plain"])
@pytest.mark.parametrize("n", SIZES)
def test_wide_io_rule(n, env):
    offs = {"llr": (0, 4, 8, 16, 20), "post": (None, 0, 4, 12, 32), "hard": (None, 0, 1, 2, 4, 7)}
    addr = lambda base, o: 0 if o is None else base + o
    grid = list(itertools.product(offs["llr"], offs["post"], offs["hard"], (0, 1), (0, 1)))
    calls = [(37, 50, algo, 0, 0, addr(BASE, l), addr(2 * BASE, p), addr(3 * BASE, h), narrow)
             for l, p, h, algo, narrow in grid]
    for (l, p, h, algo, narrow), pl in zip(grid, _plans(n, calls, env)):
        loc = pl["name"] == "bp_loc_kernel"
        want = loc and not narrow and l % 16 == 0 and (p is None or p % 16 == 0) and (h is None or h % 4 == 0)
        assert pl["wide_io"] == int(want), (n, l, p, h, algo, narrow, pl)


@pytest.mark.parametrize("n", SIZES)
def test_only_fixed_count_decodes_go_wide(n):
    calls = [(37, 50, algo, es, mc, BASE, 2 * BASE if post else 0, 3 * BASE, 0)
             for algo, es, mc, post in itertools.product((0, 1), (0, 1), (0, 1), (0, 1))]
    for c, pl in zip(calls, _plans(n, calls)):
        assert pl["wide_io"] == int(pl["name"] == "bp_loc_kernel" and not c[3] and not c[4]), (c, pl)


@pytest.mark.parametrize("env", [None, {"LDPC_NO_LOC_CHAIN": "1"}], ids=["chain", "plain"])
@pytest.mark.parametrize("n", SIZES)
def test_spare_words_and_the_first_nine_fields(n, env):
    combos = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1)))  # algo, early_stop, mc, want_post
    io = _plans(n, [(37, 50, algo, es, mc, BASE, 2 * BASE if post else 0, 3 * BASE, 0) for algo, es, mc, post in combos], env)
    with _layout_env(env):
        old = bp_plans(_csr(n), [(algo, es, mc, post, 50, 37) for algo, es, mc, post in combos])
    for c, a, b in zip(combos, io, old):
        assert {k: a[k] for k in b} == b, c
        if a["name"] == "bp_loc_kernel":
            assert a["msg_words"] >= n + 4 and a["lds"] >= 4 * a["msg_words"], (c, a)
        else:
            assert a["msg_words"] == 0 and a["wide_io"] == 0
