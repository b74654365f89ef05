"""The host-only code behind quasi-cyclic codes -- the expansion, the schedule's tables from a given
layer[] (layer_tables), the row table (csrc/graph_host.cpp) and bp_layer_q_plan's route
(csrc/bp_plan.cpp) -- compiled with tests/qc_host_main.cpp into a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer, linked against no HIP library, run as a child
process and held to the library's answers.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.qc_util import code, kernel_name, qc_plans, table_kernels
from tests.test_host_layouts import CSRC, ROOT, SAN_FLAGS

# algo, early_stop, mc, want_post, iters, B (kCalls of the program)
CALLS = [(1, 0, 0, 1, 20, 24), (1, 1, 1, 0, 20, 128), (1, 1, 0, 0, 50, 300), (1, 1, 1, 0, 40000, 128)]
FIELDS = ("name", "path", "threads", "grid", "lds", "wg_per_cu", "scratch")


@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not on the path")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path_factory.mktemp("qc_host") / "qc_host_main")
    srcs = [os.path.join(ROOT, "tests", "qc_host_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                                 ("graph_host.cpp", "loc_layout.cpp", "bp_plan.cpp")]
    subprocess.run(["g++"] + SAN_FLAGS + ["-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"),
                                          "-I" + CSRC] + srcs + ["-o", exe], check=True)
    return exe


def _run(exe, base, Z, path, *args):
    base = np.ascontiguousarray(base, np.int32)
    np.concatenate([np.array([base.shape[0], base.shape[1], Z], np.int32), base.ravel()]).tofile(path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LDPC_")}
    r = subprocess.run([exe, path] + list(args), capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    return dict(line.split("=", 1) for line in r.stdout.split())


@pytest.mark.parametrize("name", ["arr36_z7", "rnd36_z65", "hand_z31", "dense2x20_z23", "z1", "arr36_z307"])
def test_expansion_tables_and_plan_under_sanitizers(name, sanitized_program, tmp_path):
    c = code(name)
    said = _run(sanitized_program, c.base, c.Z, str(tmp_path / "base.bin"))
    cptr, cvar, vptr, vslot, layer = c.expand()
    for key, want in (("cptr", cptr), ("cvar", cvar), ("vptr", vptr), ("vslot", vslot), ("layer", layer),
                      ("cbase", np.arange(c.mb + 1) * c.Z)):
        assert [int(x) for x in said[key].split(",")] == want.tolist(), key
    d = int((c.base >= 0).sum(axis=1).max())
    assert [int(said[k]) for k in ("n", "m", "E", "max_cdeg", "lay_L", "lay_max", "block_rows", "qc_Z", "qc_mb",
                                   "qc_nb")] == [c.n, c.m, cvar.size, d, c.mb, c.Z, 1, c.Z, c.mb, c.nb]
    assert said["tables_agree"] == "1" and said["row_table_agrees"] == "1"
    plans = qc_plans(c, CALLS)
    assert said["plans"].split(";") == [":".join(str(p[k]) for k in FIELDS) for p in plans]
    assert plans[3]["name"] == "none" and plans[0]["name"] == kernel_name(c)
    # kept on the table kernels: the same schedule, no row table, bp_layer_q_kernel's plans
    table = _run(sanitized_program, c.base, c.Z, str(tmp_path / "base.bin"), "table")
    assert [int(table[k]) for k in ("lay_L", "block_rows", "qc_Z", "qc_mb", "qc_nb")] == [c.mb, 1, 0, 0, 0]
    assert table["tables_agree"] == "1" and table["row_table_agrees"] == "1" and table["layer"] == said["layer"]
    with table_kernels():
        plans = qc_plans(c, CALLS)
    assert table["plans"].split(";") == [":".join(str(p[k]) for k in FIELDS) for p in plans]
    assert plans[0]["name"].startswith("bp_layer_q_kernel<")


def test_refused_bases_under_sanitizers(sanitized_program, tmp_path):
    path = str(tmp_path / "base.bin")
    ok = [[0, 1, -1], [2, -1, 0]]
    assert "refused" not in _run(sanitized_program, ok, 3, path)
    for base, Z in ((ok, 0), (ok, 2), ([[0, -2, -1], [2, 1, 0]], 3), ([[0, 1, 2], [-1, -1, -1]], 3),
                    ([[0, -1, 1], [2, -1, 0]], 3), ([[0] * 33, [1] * 33], 2)):
        assert _run(sanitized_program, base, Z, path) == {"refused": "1"}, (base, Z)
