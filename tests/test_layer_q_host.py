"""The host-only code behind the fixed-point layered decoder -- the layer schedule's tables with the
per-layer check base (csrc/graph_host.cpp) and bp_layer_q_plan (csrc/bp_plan.cpp) -- compiled with
tests/layer_q_host_main.cpp into a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, linked against no HIP library, and held to the library's answers.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.layered_util import graph_csr, layers
from tests.layered_q_util import layer_q_plans
from tests.test_host_layouts import CSRC, ROOT, SAN_FLAGS

# algo, early_stop, mc, want_post, iters, B (kCalls of the program)
CALLS = [(1, 0, 0, 1, 20, 24), (1, 1, 1, 0, 20, 128), (1, 1, 0, 0, 50, 300), (1, 1, 1, 0, 40000, 128)]


@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not on the path")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path_factory.mktemp("layer_q_host") / "layer_q_host_main")
    srcs = [os.path.join(ROOT, "tests", "layer_q_host_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                                      ("graph_host.cpp", "loc_layout.cpp", "bp_plan.cpp")]
    subprocess.run(["g++"] + SAN_FLAGS + ["-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"),
                                          "-I" + CSRC] + srcs + ["-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name", ["r36_602", "r510_640", "mixB", "r36_5060"])
def test_check_base_and_plan_under_sanitizers(name, sanitized_program, tmp_path):
    csr = graph_csr(name)
    n, m = csr[2].size - 1, csr[0].size - 1
    path = str(tmp_path / "graph.bin")  # int32: n, m, E, check_ptr, check_var, var_ptr, var_slot
    np.concatenate([np.array([n, m, csr[1].size], np.int32)] + list(csr)).astype(np.int32).tofile(path)
    env = {k: v for k, v in os.environ.items() if k not in ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T")}
    r = subprocess.run([sanitized_program, path], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    said = dict(line.split("=", 1) for line in r.stdout.split())
    L, layer = layers(name)
    assert int(said["lay_L"]) == L and int(said["lay_max"]) == np.bincount(layer).max()
    # the check base: the number of checks in the layers before
    want = np.concatenate(([0], np.cumsum(np.bincount(layer, minlength=L))))
    assert [int(x) for x in said["cbase"].split(",")] == want.tolist()
    assert said["tables_agree"] == "1"
    plans = layer_q_plans(csr, CALLS)
    assert said["plans"].split(";") == [":".join(str(p[k]) for k in ("name", "path", "threads", "grid", "lds", "wg_per_cu",
                                                                       "scratch")) for p in plans]
    assert plans[3]["name"] == "none" and plans[0]["name"].startswith("bp_layer_q_kernel<")
