"""Host-only checks of the soft decoders' launch plan (csrc/bp_plan.cpp) through
ldpc_debug_bp_plan (no device needed): which kernel a call runs and its grid, LDS and scratch
layout, over a grid of graphs x call parameters.

tests/golden/bp_plan_parent.json holds, for the same grid, the kernel name and the scratch bytes
that the selection code and the separate sizing rule gave before the plan replaced them (run-length
coded; its "how" field says how it was dumped).  The plan
must choose the same kernel everywhere and never ask for more scratch -- except on
bp_generic_kernel<*,gmem>, where it must ask for exactly the slabs the kernel writes: the old
sizing rule gave 0 bytes to a Monte-Carlo call that a large max_iters pushes off LDS, and the
launcher refused it.
"""
import functools
import itertools
import json
import os

import numpy as np
import pytest

from iib_project_ldpc_codes_amd import ensembles
from tests.graph_util import FALLBACK_KERNELS, bp_plans, csr_from_checks, fallback_csr, regular_simple

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "bp_plan_parent.json")

# algo, early_stop, mc, want_post, iters, B
CALLS = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 50, 600), (1, 300, 70000)))
GRAPHS = ["r36_1000", "r36_4000", "r36_10000", "r36_64800", "rsu_2000", "rsu_20000", "r48_1000", "r510_1000",
          "r510_5500", "r510_8000", "deg33", "r36_10000_noloc"]
FALLBACK = ["fb_" + k for k in FALLBACK_KERNELS]  # the graphs of tests/test_gpu_fallback.py (not in the parent table)
KIB = 1024


@functools.lru_cache(maxsize=None)
def graph_csr(name):
    """((check_ptr, check_var, var_ptr, var_slot), environment of the layout build)"""
    env = {"LDPC_NO_LOC_LAYOUT": "1"} if name.endswith("_noloc") else {}
    if name.startswith("fb_"):
        return fallback_csr(name[3:]), env
    kind, n = name.split("_")[0], name.split("_")[1] if "_" in name else None
    if kind == "rsu":
        g = ensembles.sample_irregular(ensembles.RSU_DL4, int(n), seed=1, deg2="zigzag")
        return tuple(np.ascontiguousarray(a, np.int32) for a in g.to_csr()), env
    if kind == "deg33":  # check 0 holds 33 variables; checks 1..33 one of them and three more each
        rows = [np.arange(33)] + [np.array([i, 33 + 3 * i, 34 + 3 * i, 35 + 3 * i]) for i in range(33)]
        cptr = np.concatenate(([0], np.cumsum([r.size for r in rows])))
        return csr_from_checks(cptr, np.concatenate(rows), 33 + 99), env
    dv, dc = {"r36": (3, 6), "r48": (4, 8), "r510": (5, 10)}[kind]
    g = regular_simple(int(n), dv, dc, seed=1)
    return csr_from_checks(np.arange(g.m + 1) * dc, g.check_lookup, g.n), env


@functools.lru_cache(maxsize=None)
def plans(gname, cus=256):
    csr, env = graph_csr(gname)
    return bp_plans(csr, CALLS, cus=cus, env=env)


@functools.lru_cache(maxsize=None)
def parent():
    with open(GOLDEN) as f:
        graphs = json.load(f)["graphs"]
    return {g: [v["values"][i] for i, count in v["runs"] for _ in range(count)] for g, v in graphs.items()}


@pytest.mark.parametrize("gname", GRAPHS)
def test_plan_against_parent_table(gname):
    csr, _ = graph_csr(gname)
    n, E = csr[2].size - 1, csr[1].size
    rows = parent()[gname]
    assert len(rows) == len(CALLS)
    for call, p, (pname, pbytes) in zip(CALLS, plans(gname), rows):
        assert p["name"] == pname, (call, p)
        if "gmem" in p["name"]:
            assert p["scratch"] == p["grid"] * ((5 * E + 4 * n + 15) & ~15), (call, p)
        else:
            assert p["scratch"] <= pbytes, (call, p, pbytes)


def test_generic_mc_call_pushed_off_lds_gets_its_slabs():
    """(5,10) n = 5,500, Monte-Carlo, max_iters = 600: the curve pushes the messages off LDS; the
    old sizing rule gave this call no scratch at all."""
    hit = 0
    for call, p, (pname, pbytes) in zip(CALLS, plans("r510_5500"), parent()["r510_5500"]):
        algo, early_stop, mc, want_post, iters, B = call
        if mc and iters == 600:
            assert p["name"] == "bp_generic_kernel<16,gmem>" and pbytes == 0 and p["scratch"] > 0, (call, p)
            hit += 1
    assert hit == 2 * 2 * 2 * 3


@pytest.mark.parametrize("gname", GRAPHS + FALLBACK)
def test_plan_invariants(gname):
    for call, p in zip(CALLS, plans(gname)):
        B = call[5]
        if p["name"] == "none":
            assert gname == "deg33"
            continue
        assert 1 <= p["grid"] <= B, (call, p)
        assert p["lds"] <= 160 * KIB, (call, p)
        assert p["threads"] in (256, 512, 1024), (call, p)
        assert bool(p["persistent"]) == (p["counter"] >= 0), (call, p)
        if p["counter"] >= 0:
            assert p["counter"] + 4 <= p["scratch"] and p["slab"] <= p["counter"], (call, p)
        else:
            assert p["slab"] <= p["scratch"], (call, p)
    assert gname != "deg33" or all(p["name"] == "none" for p in plans(gname))


@pytest.mark.parametrize("name", list(FALLBACK_KERNELS))
def test_fallback_graphs_run_the_kernels_their_gpu_tests_name(name):
    """Every call shape of tests/test_gpu_fallback.py: plain decodes of 24 / 32 / 264 frames up to 20
    iterations and 20-iteration Monte-Carlo batches of 128, both algorithms, with and without
    early stop.  The slab forms really keep messages in the slab (0 < lds_slots < E, or irr_S <
    irr_P behind the <lds+slab> name) and cap the grid at one workgroup per CU."""
    csr = fallback_csr(name)
    E = csr[1].size
    calls = [(algo, es, 0, 1, it, B) for algo in (0, 1) for es in (0, 1) for it in (1, 3, 5, 10, 20) for B in (24, 32, 264)]
    calls += [(algo, es, 1, 0, 20, 128) for algo in (0, 1) for es in (0, 1)]
    want = FALLBACK_KERNELS[name]
    for call, p in zip(calls, bp_plans(csr, calls)):
        assert p["name"] == want, (call, p)
        if "gmem" in want or "slab" in want:
            assert p["grid"] == min(call[5], 256) and p["slab"] > 0, (call, p)
        else:
            assert p["grid"] == call[5] and p["scratch"] == 0, (call, p)
        if "gmem" in want:
            assert 0 < p["lds_slots"] < E, (call, p)
            assert p["scratch"] == p["grid"] * ((5 * E + 4 * (csr[2].size - 1) + 15) & ~15), (call, p)


@pytest.mark.parametrize("gname", ["r36_1000", "r36_10000", "rsu_2000"])
def test_persistent_grid_follows_the_cu_count(gname):
    seen = 0
    for call, p, p8 in zip(CALLS, plans(gname), plans(gname, 8)):
        B = call[5]
        assert p8["name"] == p["name"] and p8["persistent"] == p["persistent"]
        if p["persistent"]:
            assert p["grid"] == min(B, 512) and p8["grid"] == min(B, 16), (call, p, p8)
            seen += 1
        else:
            assert p8["grid"] == p["grid"] and p8["scratch"] == p["scratch"], (call, p, p8)
    assert seen


def test_names_the_gpu_tests_pin():
    csr, _ = graph_csr("r36_10000")
    # as ldpc_bp_kernel_name asks: sum-product, 50 iterations, with and without posteriors
    assert [p["name"] for p in bp_plans(csr, [(0, 1, 0, 0, 50, 1), (0, 1, 0, 1, 50, 1)])] == ["bp_loc_kernel"] * 2
    csr, _ = graph_csr("r36_1000")
    assert bp_plans(csr, [(1, 0, 0, 1, 50, 64)])[0]["name"] == "bp_lds_kernel<3,6>"
