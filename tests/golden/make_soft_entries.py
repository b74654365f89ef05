"""Record soft_entries_parent.json: what the soft decoders' entry points answer on the inputs of
tests/test_gpu_soft_entries.py (its record()).  Run on an MI355X, with the library built, at the
commit whose answers are to be pinned -- the committed file is from the parent of the commit that
brought SoftCall and the two drivers into csrc/capi.cpp:

    python tests/golden/make_soft_entries.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import test_gpu_soft_entries as t  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "soft_entries_parent.json")
    inputs = {"n": t.N, "dv": t.DV, "dc": t.DC, "B": t.B, "max_iters": t.ITERS, "seed": t.SEED, "alpha": t.ALPHA,
              "bec": t.PARAM[t.BEC], "bsc": t.PARAM[t.BSC], "awgn": t.PARAM[t.AWGN]}
    with open(out, "w") as f:
        json.dump({"inputs": inputs, "calls": t.record(t.Env())}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)
