"""The per-codeword fixed cost of the fixed-count sum-product decode on the bench workload
((3,6) n = 10,000 seed 1, B = 65,536 frames at sigma = 0.85, the frames bench.py decodes): the
launch time at 10, 20, 30, 40 and 50 iterations (HIP events, the median of 7 launches after 2
warm-up launches), and the least-squares line t = a + b iters through them.  b is one
iteration of the whole batch, a what a codeword costs outside the iteration loop (staging,
posteriors, outputs), in ms per launch; a / b is that cost in iterations.
    python scripts/loc_fixed_cost.py --label new [--out profiles/loc_fixed_cost.json]
(LDPC_LIB_PATH selects the library, as in scripts/ab_decode.sh; --out adds or replaces the row
of this label in the file.)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from iib_project_ldpc_codes_amd import decoder
from iib_project_ldpc_codes_amd.graph import TannerGraph

ITERS = (10, 20, 30, 40, 50)
WARMUP, REPS = 2, 7

ap = argparse.ArgumentParser()
ap.add_argument("--label", required=True)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--sigma", type=float, default=0.85)
ap.add_argument("--out", default=None)
a = ap.parse_args()

g = TannerGraph.random_regular(10000, 3, 6, seed=1)
llr = decoder.channel_dev("awgn", a.sigma, 2026, 0, g.n, a.batch)
s = torch.cuda.current_stream()
ms = []
for iters in ITERS:
    ts = []
    for r in range(WARMUP + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        decoder.bp_decode_dev(g, llr, iters, "spa", 1.0, False, stream=s, want_post=True)
        e1.record(s)
        torch.cuda.synchronize()
        if r >= WARMUP:
            ts.append(e0.elapsed_time(e1))
    ms.append(float(np.median(ts)))
b_fit, a_fit = np.polyfit(np.array(ITERS, float), np.array(ms), 1)
resid = np.array(ms) - (a_fit + b_fit * np.array(ITERS, float))
row = {"label": a.label, "kernel": g.kernel_name(), "batch": a.batch, "sigma": a.sigma, "iters": list(ITERS),
       "median_ms": [round(t, 4) for t in ms], "a_ms": round(float(a_fit), 4), "b_ms_per_iter": round(float(b_fit), 5),
       "a_in_iterations": round(float(a_fit / b_fit), 3), "max_abs_residual_ms": round(float(np.abs(resid).max()), 4)}
print(json.dumps(row), flush=True)
if a.out:
    rows = []
    if os.path.exists(a.out):
        with open(a.out) as f:
            rows = [r for r in json.load(f)["rows"] if r["label"] != a.label]
    with open(a.out, "w") as f:
        json.dump({"what": "scripts/loc_fixed_cost.py: launch time t = a + b iters of the fixed-count sum-product "
                           "decode on the bench workload (ms per launch of the whole batch)",
                   "rows": rows + [row]}, f, indent=1)
        f.write("\n")
