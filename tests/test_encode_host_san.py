"""The host-only code behind the encoder -- the elimination and the device tables
(csrc/encode_host.cpp) and encode_plan (csrc/encode_plan.cpp) -- compiled with
tests/encode_host_main.cpp into a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, linked against no HIP library, and held to the library's answers.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import encode_util as eu
from tests.test_host_layouts import CSRC, ROOT, SAN_FLAGS

BATCHES = (1, 33, 257, 65536)  # kBatches of the program


@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not on the path")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path_factory.mktemp("encode_host") / "encode_host_main")
    srcs = [os.path.join(ROOT, "tests", "encode_host_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                                     ("encode_host.cpp", "encode_plan.cpp")]
    subprocess.run(["g++"] + SAN_FLAGS + ["-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"),
                                          "-I" + CSRC] + srcs + ["-o", exe], check=True)
    return exe


def _ints(text):
    return [] if text == "-" else [int(x) for x in text.split(",")]


@pytest.mark.parametrize("name", eu.NAMES)
def test_elimination_and_plan_under_sanitizers(name, sanitized_program, tmp_path):
    cptr, cvar, n = eu.graph(name)
    path = str(tmp_path / "graph.bin")  # int32: n, m, E, check_ptr, check_var
    np.concatenate([np.array([n, cptr.size - 1, cvar.size], np.int32), cptr, cvar]).astype(np.int32).tofile(path)
    r = subprocess.run([sanitized_program, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    said = dict(line.split("=", 1) for line in r.stdout.split())
    rank, info, par, A = eu.description(name)
    K = n - rank
    assert (int(said["n"]), int(said["rank"]), int(said["K"]), int(said["KW"])) == (n, rank, K, (K + 31) // 32)
    assert _ints(said["info"]) == info.tolist() and _ints(said["par"]) == par.tolist()
    assert _ints(said["A"]) == A.ravel().tolist()
    assert said["tables_agree"] == "1"
    rc, rows = eu.encode_plans([(n, K, rank, B) for B in BATCHES])
    assert rc == 0
    assert said["plans"].split(";") == [":".join(str(p[k]) for k in ("name", "threads", "W", "grid", "lds", "scratch",
                                                                       "write_grid")) for p in rows]
