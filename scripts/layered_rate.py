"""The layered (row-serial) schedule against the flooding one: rate, iterations and frame errors.

Times, in one process on one device, with HIP events (warm-up launches, then the median of
--launches timed ones, the same device-resident frames every launch):
  (a) the headline code, (3,6) n = 10,000, B = 16,384 BI-AWGN frames at sigma = 0.85, early stop,
      at most 50 iterations, hard decisions only, normalized min-sum (alpha 0.75) and sum-product:
      bp_layer_kernel against the flooding decode of the same call (bp_loc_kernel) -- codewords/s,
      mean iterations, frame errors;
  (b) the same frames at a fixed count of 10 and of 20 iterations: the frame errors of both
      schedules (what an iteration-limited decoder reaches);
  (c) r510_9000 ((5,10) n = 9,000), where flooding runs bp_generic_kernel<16,gmem>, the nearest
      like-for-like kernel: time per iteration of a fixed-count decode of both.
Writes the numbers as JSON.

  python scripts/layered_rate.py [--out profiles/layered_rate.json] [--launches 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from iib_project_ldpc_codes_amd import decoder  # noqa: E402
from iib_project_ldpc_codes_amd.graph import TannerGraph  # noqa: E402

SIGMA, SEED, ITERS, ALPHA = 0.85, 2026, 50, 0.75
ALGOS = (("minsum", ALPHA), ("spa", 1.0))
SCHEDULES = ("layered", "flooding")


def timed(launch, warmup, launches):
    """Milliseconds of launch(): warm-up launches untimed, then one event pair each."""
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        launch()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms


def summary(ms, B):
    med = statistics.median(ms)
    return {"launch_ms_median": med, "launch_ms_min": min(ms), "launch_ms_max": max(ms), "launches": len(ms),
            "codewords_per_s": B / (med * 1e-3)}


def r510_9000():
    """tests/graph_util.py's graph of that name (regular_simple(9000, 5, 10, seed=1)), restated
    so the script needs nothing of the test tree."""
    rng = np.random.default_rng(1)
    n, dv, dc = 9000, 5, 10
    E, m = n * dv, n * dv // dc
    chk = np.arange(E) // dc
    cvar = np.repeat(np.arange(n, dtype=np.int32), dv)[rng.permutation(E)]
    for _ in range(1000):
        key = chk.astype(np.int64) * n + cvar
        order = np.argsort(key, kind="stable")
        dup = order[1:][key[order][1:] == key[order][:-1]]
        if not dup.size:
            break
        for s in dup:
            t = rng.integers(E)
            cvar[s], cvar[t] = cvar[t], cvar[s]
    var = chk[np.lexsort((chk, cvar))].astype(np.int32)
    return TannerGraph(var, cvar, n, n - m, dv, dc)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "layered_rate.json"))
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch sizes (a quick run)")
    args = ap.parse_args(argv)
    assert args.launches >= 5
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "sigma": SIGMA, "seed": SEED, "alpha_minsum": ALPHA,
           "layer_rule": decoder.layer_rule(), "launches": args.launches, "warmup": args.warmup}

    # (a), (b): the headline code
    g = TannerGraph.random_regular(10000, 3, 6, seed=1)
    B = 16384 // args.scale
    llr = decoder.channel_dev("awgn", SIGMA, SEED, 0, g.n, B)
    hard = torch.empty((B, g.n), dtype=torch.uint8, device="cuda")
    its = torch.empty((B,), dtype=torch.int32, device="cuda")
    layers = g.layer_schedule()
    head = {"n": g.n, "dv": 3, "dc": 6, "batch": B, "layers": int(layers.max()) + 1,
            "largest_layer": int(np.bincount(layers).max()),
            "flooding_kernel": g.kernel_name(early_stop=True, hard_only=True), "early_stop": {}, "fixed_count": {}}
    for algo, alpha in ALGOS:
        for sched in SCHEDULES:
            def run(iters=ITERS, es=True):
                decoder.bp_decode_dev(g, llr, iters, algo, alpha, es, hard=hard, its=its, want_post=False,
                                      schedule=sched)
            row = summary(timed(run, args.warmup, args.launches), B)
            row["max_iters"] = ITERS
            row["mean_iterations"] = float(its.float().mean())
            row["frame_errors"] = int(hard.any(dim=1).sum())
            head["early_stop"]["%s_%s" % (algo, sched)] = row
            print("a", algo, sched, json.dumps(row), flush=True)
            for iters in (10, 20):
                run(iters, False)
                torch.cuda.synchronize()
                head["fixed_count"]["%s_%s_%d" % (algo, sched, iters)] = {"frame_errors": int(hard.any(dim=1).sum())}
        e = head["early_stop"]
        e["%s_layered_over_flooding" % algo] = (e["%s_layered" % algo]["codewords_per_s"] /
                                                e["%s_flooding" % algo]["codewords_per_s"])
    print("b", json.dumps(head["fixed_count"]), flush=True)
    out["headline"] = head
    del llr, hard, its

    # (c): time per iteration on the nearest like-for-like flooding kernel
    g = r510_9000()
    B, iters = 4096 // args.scale, 20
    llr = decoder.channel_dev("awgn", SIGMA, SEED, 0, g.n, B)
    hard = torch.empty((B, g.n), dtype=torch.uint8, device="cuda")
    its = torch.empty((B,), dtype=torch.int32, device="cuda")
    like = {"n": g.n, "dv": 5, "dc": 10, "batch": B, "iterations": iters, "flooding_kernel": g.kernel_name()}
    for algo, alpha in ALGOS:
        for sched in SCHEDULES:
            def run():
                decoder.bp_decode_dev(g, llr, iters, algo, alpha, False, hard=hard, its=its, want_post=False,
                                      schedule=sched)
            row = summary(timed(run, args.warmup, args.launches), B)
            row["us_per_codeword_iteration"] = row["launch_ms_median"] * 1e3 / (B * iters)
            like["%s_%s" % (algo, sched)] = row
            print("c", algo, sched, json.dumps(row), flush=True)
    out["r510_9000"] = like
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
