"""Host-only checks of the chained local-edge layout (csrc/loc_layout.cpp, build_loc_chain_layout)
through ldpc_debug_loc_chain_layout (no device needed).

On (3,6) graphs at the 512 x 5 shape (n = 4,100: the smallest, a part-filled wave and wholly idle
waves; n = 10,000 seed 1: the bench code; n = 10,200: the largest that fits):
  * every variable has exactly one local edge and every check exactly two;
  * every edge is exactly one of local, chain or LDS: n local, 8 Tq chain, 32 Tq LDS;
  * LDS words are distinct and below `words`;
  * for each thread, half and k < CL the chain edge of var pair 2k + 1 goes to the check at pair
    slot k + 1, same half, same thread;
  * float4 / float2 rows are 16- / 8-byte aligned;
  * two builds give identical tables.
A graph whose pair count is no multiple of 5, or with a repeated variable in a check, has no
chained layout and still answers the plain one.
"""
import functools

import numpy as np
import pytest

from iib_project_ldpc_codes_amd import _native
from iib_project_ldpc_codes_amd.graph import TannerGraph
from tests.graph_util import csr_from_checks

T, KP, CL, DVN = 512, 5, 4, 2


def csr_of(n, seed=1):
    g = TannerGraph.random_regular(n, 3, 6, seed=seed)
    return csr_from_checks(np.arange(g.m + 1) * 6, np.ascontiguousarray(g.check_lookup, np.int32), g.n)


def chain_layout(csr):
    ptrs = [a.ctypes.data for a in csr]
    n, m = csr[2].size - 1, csr[0].size - 1
    shape = np.zeros(6, np.int32)
    var, pos = np.zeros(2 * KP * 2 * T, np.int32), np.zeros(2 * KP * DVN * T, np.int32)
    info, chk = np.zeros(2 * KP * T, np.int32), np.zeros(2 * KP * T, np.int32)
    rc = _native.lib().ldpc_debug_loc_chain_layout(*ptrs, n, m, shape.ctypes.data, var.ctypes.data, pos.ctypes.data,
                                                   info.ctypes.data, chk.ctypes.data)
    return rc, shape, var.reshape(2 * KP, 2, T), pos.reshape(2 * KP, DVN, T), info.reshape(2 * KP, T), \
        chk.reshape(KP, 2, T)


def plain_layout(csr):
    ptrs = [a.ctypes.data for a in csr]
    n, m = csr[2].size - 1, csr[0].size - 1
    shape = np.zeros(24, np.int32)
    rc = _native.lib().ldpc_debug_loc_layout(*ptrs, n, m, T, shape.ctypes.data, None, None, None)
    return rc, shape


@functools.lru_cache(maxsize=None)
def built(n):
    csr = csr_of(n)
    return csr, chain_layout(csr)


def word_owner(w, Tq):
    """(pair slot k, thread, half, LDS input u) of LDS word w"""
    if w < 8 * Tq:  # pair slot 0: two float4 rows
        r, x = divmod(w, 4 * Tq)
        t, y = divmod(x, 4)
        return 0, t, y % 2, 2 * r + y // 2
    w -= 8 * Tq
    if w < 16 * Tq:  # pair slots >= 1: the float4 row
        i, y = divmod(w, 4)
        return 1 + i // Tq, i % Tq, y % 2, y // 2
    i, h = divmod(w - 16 * Tq, 2)  # the float2 row
    return 1 + i // Tq, i % Tq, h, 2


@pytest.mark.parametrize("n", [4100, 10000, 10200])
def test_chain_layout_covers_the_graph(n):
    csr, (rc, shape, var, pos, info, chk) = built(n)
    cptr, cvar, vptr, vslot = csr
    m = cptr.size - 1
    assert rc == 0, _native.last_error()
    Tq, words = int(shape[0]), int(shape[3])
    assert (Tq, int(shape[1]), int(shape[2]), words, int(shape[5])) == (m // 2 // KP, KP, CL, 32 * m // 2 // KP, T)
    # float4 rows from words 0, 4 Tq, 8 Tq, the float2 row from word 24 Tq: 16- / 8-byte aligned
    assert (4 * Tq * 4) % 16 == 0 and (8 * Tq * 4) % 16 == 0 and (24 * Tq * 4) % 8 == 0
    # threads >= Tq own nothing; the others' checks partition the checks
    assert (chk[:, :, Tq:] == -1).all() and (var[:, :, Tq:] == -1).all()
    assert np.array_equal(np.sort(chk[:, :, :Tq].ravel()), np.arange(m))
    # every variable is local exactly once, every check holds exactly two local variables
    assert np.array_equal(np.sort(var[:, :, :Tq].ravel()), np.arange(n))
    slot_check = np.repeat(np.arange(m), 6)
    holds = [set(cvar[6 * c:6 * c + 6]) for c in range(m)]
    kind = np.full(cvar.size, -1)  # per check-major edge slot: 0 local, 1 chain, 2 LDS
    seen_words = np.zeros(words, bool)
    counts = [0, 0, 0]
    for t in range(Tq):
        for k in range(KP):
            for h in range(2):
                c = int(chk[k, h, t])
                for s in range(2):
                    vi = 2 * k + s
                    v = int(var[vi, h, t])
                    assert v in holds[c]
                    edges = [int(vslot[e]) for e in range(vptr[v], vptr[v + 1])]
                    local = [e for e in edges if slot_check[e] == c]
                    assert len(local) == 1
                    rest = [e for e in edges if slot_check[e] != c]
                    chained = s == 1 and k < CL
                    nl = 1 if chained else 2
                    assert (int(info[vi, t]) >> (4 * h)) & 15 == (1 << nl) - 1
                    if chained:  # the chain edge goes to the check at pair slot k + 1, same half and thread
                        nxt = int(chk[k + 1, h, t])
                        to_next = [e for e in rest if slot_check[e] == nxt]
                        assert len(to_next) == 1
                        assert kind[to_next[0]] == -1
                        kind[to_next[0]] = 1
                        counts[1] += 1
                        rest = [e for e in rest if e != to_next[0]]
                    assert kind[local[0]] == -1
                    kind[local[0]] = 0
                    counts[0] += 1
                    for u, e in enumerate(rest):  # LDS edges in variable_to_check_list order
                        w = (int(pos[vi, u, t]) >> (16 * h)) & 0xFFFF
                        assert w < words and not seen_words[w]
                        seen_words[w] = True
                        k2, t2, h2, u2 = word_owner(w, Tq)
                        assert int(chk[k2, h2, t2]) == slot_check[e] and u2 < (4 if k2 == 0 else 3)
                        assert kind[e] == -1
                        kind[e] = 2
                        counts[2] += 1
    assert counts == [n, 8 * Tq, 32 * Tq]
    assert (kind >= 0).all() and seen_words.all()
    # per check: two local edges, one chain input at pair slots >= 1, the rest in LDS
    per = kind.reshape(m, 6)
    assert ((per == 0).sum(1) == 2).all()
    slot_k = np.zeros(m, int)
    for k in range(KP):
        slot_k[chk[k, :, :Tq].ravel()] = k
    assert np.array_equal((per == 1).sum(1), (slot_k > 0).astype(int))
    # threads without variables and the unused row of a chained var pair: dummy words after the messages
    idle = pos[:, :, Tq:].astype(np.int64) & 0xFFFFFFFF
    assert ((idle & 0xFFFF) >= words).all() and ((idle & 0xFFFF) < words + 64).all()
    assert ((idle >> 16) >= words).all() and ((idle >> 16) < words + 64).all()
    spare = pos[1:2 * CL:2, 1, :Tq].astype(np.int64) & 0xFFFF
    assert (spare >= words).all() and (spare < words + 64).all()


@pytest.mark.parametrize("n", [4100, 10000, 10200])
def test_chain_layout_is_deterministic(n):
    csr, first = built(n)
    again = chain_layout(csr)
    assert again[0] == first[0] == 0
    for a, b in zip(first[1:], again[1:]):
        assert np.array_equal(a, b)


def test_plan_sizes_lds_from_the_chained_layout(monkeypatch):
    """Fixed-count sum-product on the bench code: 16,000 + 64 message words instead of 20,000 + 64;
    every other mode, and LDPC_NO_LOC_CHAIN=1, keep the plain layout's plan."""
    from tests.graph_util import bp_plans
    csr, _ = built(10000)
    calls = [(0, 0, 0, 1, 50, 300), (1, 0, 0, 1, 50, 300), (0, 1, 0, 0, 50, 300), (0, 0, 1, 0, 50, 300)]
    monkeypatch.delenv("LDPC_NO_LOC_CHAIN", raising=False)
    on = bp_plans(csr, calls)
    monkeypatch.setenv("LDPC_NO_LOC_CHAIN", "1")
    off = bp_plans(csr, calls)
    assert all(p["name"] == "bp_loc_kernel" for p in on + off)
    assert on[0]["lds"] == 4 * (16000 + 64) and off[0]["lds"] == 4 * (20000 + 64)
    assert on[1:] == off[1:]
    assert {k: v for k, v in on[0].items() if k != "lds"} == {k: v for k, v in off[0].items() if k != "lds"}


def test_pair_count_not_a_multiple_of_five_has_no_chain():
    csr = csr_of(4104)  # P = 1,026
    assert chain_layout(csr)[0] == _native.LDPC_EUNSUP
    rc, shape = plain_layout(csr)
    assert rc == 0 and (int(shape[0]), int(shape[1]), int(shape[3])) == (T, KP, 1026)


def test_repeated_variable_in_a_check_has_no_chain():
    cptr, cvar, _, _ = csr_of(4100)
    cvar = cvar.copy()
    # check 0 swaps its second variable for another check's copy of its first: the degrees stay
    # (3, 6), and check 0 now holds one variable twice
    src = next(i for i in range(6, cvar.size) if cvar[i] == cvar[0] and cvar[1] not in cvar[i - i % 6:i - i % 6 + 6])
    cvar[1], cvar[src] = cvar[src], cvar[1]
    assert cvar[0] == cvar[1]
    csr = csr_from_checks(cptr, cvar, 4100)
    assert chain_layout(csr)[0] == _native.LDPC_EUNSUP
    rc, shape = plain_layout(csr)
    assert rc == 0 and (int(shape[0]), int(shape[1]), int(shape[3])) == (T, KP, 1025)
