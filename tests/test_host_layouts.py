"""Host-only checks of graph preparation (csrc/graph_host.cpp): the layouts the soft decoders run
on, read through the ldpc_debug_* entries (no device needed), are bit-identical to
tests/golden/host_layouts_parent.json -- return codes, shape scalars and a SHA-256 of every output
array, recorded before graph preparation moved out of the C ABI file (its "how" field says how).
Every graph is measured with the layout environment unset, with LDPC_NO_LOC_LAYOUT=1 and with
LDPC_LOC_T set: only ldpc_debug_loc_variant and ldpc_debug_bp_plan may answer differently.

test_host_layouts_under_sanitizers compiles the same host code (graph_host.cpp, loc_layout.cpp,
bp_plan.cpp) with tests/host_layouts_main.cpp as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, linked against no HIP library, and compares what it prints with the
library's answers.
"""
import ctypes as ct
import functools
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from iib_project_ldpc_codes_amd import _native, ensembles
from tests.graph_util import bp_plans, check6_var24, csr_from_checks, regular_simple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_layouts_parent.json")
GRAPHS = ["r36_96", "r36_1000", "r36_4000", "r48_1000", "r510_1000", "rsu_2000", "check6var24_500", "deg33",
          "r36_96_repeated"]
ENVS = {"default": {}, "noloc": {"LDPC_NO_LOC_LAYOUT": "1"}, "loct": {"LDPC_LOC_T": "1024"}}
LOC_T = (256, 512, 1024)
# algo, early_stop, mc, want_post, iters, B
PLAN_CALLS = [(0, 0, 0, 1, 50, 300), (1, 0, 0, 1, 50, 300), (0, 1, 0, 0, 50, 300), (0, 1, 0, 1, 50, 70000),
              (1, 1, 1, 0, 50, 300), (0, 0, 1, 0, 600, 300)]


@functools.lru_cache(maxsize=None)
def graph(name):
    """(lists or None, csr or None): lists = (variable_to_check, check_to_variable, n, k, dv, dc)"""
    kind, n = name.split("_")[0], int(name.split("_")[1]) if "_" in name else 0
    if kind == "rsu":
        g = ensembles.sample_irregular(ensembles.RSU_DL4, n, seed=1, deg2="zigzag")
        return None, tuple(np.ascontiguousarray(a, np.int32) for a in g.to_csr())
    if kind == "check6var24":
        return None, tuple(np.ascontiguousarray(a, np.int32) for a in check6_var24(n).to_csr())
    if kind == "deg33":  # as tests/test_bp_plan.py: check 0 holds 33 variables
        rows = [np.arange(33)] + [np.array([i, 33 + 3 * i, 34 + 3 * i, 35 + 3 * i]) for i in range(33)]
        cptr = np.concatenate(([0], np.cumsum([r.size for r in rows])))
        return None, csr_from_checks(cptr, np.concatenate(rows), 33 + 99)
    dv, dc = {"r36": (3, 6), "r48": (4, 8), "r510": (5, 10)}[kind]
    g = regular_simple(n, dv, dc, seed=1)
    v2c = np.ascontiguousarray(g.variable_lookup, np.int32)
    c2v = np.ascontiguousarray(g.check_lookup, np.int32).copy()
    if name.endswith("_repeated"):
        # check 0 lists its first variable twice (in place of its second): the pair (v, 0) is
        # repeated on the check side only, so the lists are not consistent
        c2v[1] = c2v[0]
        return (v2c, c2v, g.n, g.k, dv, dc), None
    return (v2c, c2v, g.n, g.k, dv, dc), csr_from_checks(np.arange(g.m + 1) * dc, c2v, g.n)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.int32).tobytes()).hexdigest()


def lane_layout(lists):
    v2c, c2v, n, k, dv, dc = lists
    L = _native.lib()
    T, V = ct.c_int32(), ct.c_int32()
    rc = L.ldpc_debug_lane_layout(v2c.ctypes.data, c2v.ctypes.data, n, k, dv, dc, ct.byref(T), ct.byref(V), None, None)
    if rc:
        return {"rc": rc}
    lv, ls = np.zeros(T.value * V.value, np.int32), np.zeros(T.value * V.value * dv, np.int32)
    rc = L.ldpc_debug_lane_layout(v2c.ctypes.data, c2v.ctypes.data, n, k, dv, dc, ct.byref(T), ct.byref(V),
                                  lv.ctypes.data, ls.ctypes.data)
    return {"rc": rc, "T": T.value, "VPT": V.value, "lane_var": sha(lv), "lane_slot": sha(ls)}


def irr_layout(csr):
    ptrs = [a.ctypes.data for a in csr]
    n, m = csr[2].size - 1, csr[0].size - 1
    L = _native.lib()
    shape = np.zeros(5, np.int32)
    rc = L.ldpc_debug_irr_layout(*ptrs, n, m, shape.ctypes.data, None, None)
    if rc:
        return {"rc": rc}
    lane, cdeg = np.zeros(3 * 1024 * int(shape[0]), np.int32), np.zeros(2 * 1024, np.int32)
    rc = L.ldpc_debug_irr_layout(*ptrs, n, m, shape.ctypes.data, lane.ctypes.data, cdeg.ctypes.data)
    return {"rc": rc, "shape": shape.tolist(), "lane": sha(lane), "cdeg": sha(cdeg)}


def loc_layout(csr, T):
    ptrs = [a.ctypes.data for a in csr]
    n, m = csr[2].size - 1, csr[0].size - 1
    L = _native.lib()
    shape = np.zeros(24, np.int32)
    rc = L.ldpc_debug_loc_layout(*ptrs, n, m, T, shape.ctypes.data, None, None, None)
    if rc:
        return {"rc": rc}
    VP, D = 2 * int(shape[1]), max(int(shape[2]), 1)
    var, pos, info = np.zeros(VP * 2 * T, np.int32), np.zeros(VP * D * T, np.int32), np.zeros(VP * T, np.int32)
    rc = L.ldpc_debug_loc_layout(*ptrs, n, m, T, shape.ctypes.data, var.ctypes.data, pos.ctypes.data, info.ctypes.data)
    return {"rc": rc, "shape": shape.tolist(), "var": sha(var), "pos": sha(pos), "info": sha(info)}


def loc_variant(csr, T):
    out = np.zeros(1, np.int32)
    rc = _native.lib().ldpc_debug_loc_variant(*[a.ctypes.data for a in csr], csr[2].size - 1, csr[0].size - 1, T,
                                              out.ctypes.data)
    return {"rc": rc, "variant": int(out[0])}


def measure(name, env):
    """Everything the host-only entries say about one graph, with `env` as the layout environment
    (set and restored as graph_util.bp_plans does)."""
    lists, csr = graph(name)
    saved = {k: os.environ.pop(k, None) for k in ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T")}
    os.environ.update(env)
    try:
        out = {}
        if lists:
            out["lane"] = lane_layout(lists)
        if csr:
            out["irr"] = irr_layout(csr)
            out["loc"] = {str(T): loc_layout(csr, T) for T in LOC_T}
            out["variant"] = {str(T): loc_variant(csr, T) for T in LOC_T}
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    if csr:  # bp_plans sets the environment itself
        # kernel and threads only: where LDPC_LOC_T shows (tests/test_bp_plan.py holds the sizes)
        out["plans"] = [[p["name"], p["threads"]] for p in bp_plans(csr, PLAN_CALLS, env=env)]
    return out


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["graphs"]


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("name", GRAPHS)
def test_layouts_equal_the_parents(name, env):
    want = golden()[name]
    got = measure(name, ENVS[env])
    for key in ("lane", "irr", "loc"):  # the environment never reaches these
        assert got.get(key) == want["layouts"].get(key), key
    for key in ("variant", "plans"):
        assert got.get(key) == want[env].get(key), key


def test_golden_covers_the_branches():
    """The recorded parent took the branches the graphs were chosen for."""
    g = golden()
    assert g["r36_1000"]["layouts"]["lane"]["T"] == 256 and g["r36_4000"]["layouts"]["lane"]["T"] == 1024
    assert g["r48_1000"]["layouts"]["irr"]["shape"][2] == 8  # DC
    assert g["r510_1000"]["layouts"]["irr"]["rc"] == _native.LDPC_EUNSUP
    assert g["r36_96_repeated"]["layouts"]["lane"] == {"rc": _native.LDPC_EINVAL}
    assert g["r36_1000"]["default"]["variant"]["256"]["variant"] == 1
    assert g["r36_1000"]["noloc"]["variant"]["256"]["variant"] == 0
    assert g["rsu_2000"]["default"]["variant"]["256"]["variant"] == 2
    assert g["check6var24_500"]["default"]["variant"]["256"]["variant"] == 2
    assert g["r36_1000"]["default"]["plans"] != g["r36_1000"]["loct"]["plans"]
    assert all(p[0] == "none" for p in g["deg33"]["default"]["plans"])


# ---- the same host code as a stand-alone program under ASan + UBSan ------------------------------
CSRC = os.path.join(ROOT, "iib_project_ldpc_codes_amd", "csrc")
# the sanitizer runtimes linked statically: the program starts whatever else the loader brings in first
SAN_FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-D__HIP_PLATFORM_AMD__", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not on the path")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path_factory.mktemp("host_layouts") / "host_layouts_main")
    srcs = [os.path.join(ROOT, "tests", "host_layouts_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                                       ("graph_host.cpp", "loc_layout.cpp", "bp_plan.cpp")]
    # no HIP library on the link line: graph preparation and the launch plan are host-only
    subprocess.run(["g++"] + SAN_FLAGS + ["-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"),
                                          "-I" + CSRC] + srcs + ["-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name", ["r36_1000", "rsu_2000", "r48_1000"])
def test_host_layouts_under_sanitizers(name, sanitized_program, tmp_path):
    csr = graph(name)[1]
    n, m = csr[2].size - 1, csr[0].size - 1
    path = str(tmp_path / "graph.bin")  # int32: n, m, E, check_ptr, check_var, var_ptr, var_slot
    np.concatenate([np.array([n, m, csr[1].size], np.int32)] + list(csr)).astype(np.int32).tofile(path)
    env = {k: v for k, v in os.environ.items() if k not in ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T")}
    r = subprocess.run([sanitized_program, path], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    said = dict(line.split("=", 1) for line in r.stdout.split())
    want = golden()[name]
    irr, loc = want["layouts"]["irr"], want["layouts"]["loc"]
    lane_T, irr_VPT = int(said["lane_T"]), int(said["irr_VPT"])
    if lane_T:
        lists = graph(name)[0]
        lane = lane_layout(lists)
        assert (lane_T, int(said["lane_VPT"])) == (lane["T"], lane["VPT"])
    else:  # the irregular layout is built when there is no lane layout
        assert irr["rc"] == 0
        assert [int(said[k]) for k in ("irr_VPT", "irr_KC", "irr_DC", "irr_S", "irr_P")] == irr["shape"]
    assert bool(lane_T) != bool(irr_VPT)
    shape = loc[said["loc_T"]]["shape"]  # T, KP, DVN, P, words, ncls
    assert [int(said[k]) for k in ("loc_T", "loc_KP", "loc_DVN", "loc_P", "loc_words", "loc_ncls")] == shape[:6]
    assert (int(said["loc_dvn0"]), int(said["loc_dvn1"])) == (shape[22] & 255, shape[23] & 255)
    assert int(said["variant"]) == loc_variant(csr, int(said["loc_T"]))["variant"]
    assert int(said["off_loc_KP"]) == 0 and int(said["off_lane_T"]) == lane_T and int(said["off_irr_VPT"]) == irr_VPT
    plans = bp_plans(csr, PLAN_CALLS)
    assert said["plans"].split(";") == [p["name"] for p in plans]
    assert said["off_plans"].split(";") == [p["name"] for p in bp_plans(csr, PLAN_CALLS, env=ENVS["noloc"])]
    assert [int(x) for x in said["scratch"].split(",")] == [p["scratch"] for p in plans]
