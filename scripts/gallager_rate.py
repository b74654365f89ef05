"""Gallager A Monte-Carlo (ldpc_mc_gb_batch_dev, b = 0) against the min-sum Monte-Carlo
(ldpc_mc_batch_dev, alpha = 0.75) on the same code, channel and trials: rate, iterations, frame errors.

(3,6) n = 10,000 (the cfg3 code of scripts/fer_sweep.py), BSC at p = 0.030 and 0.038, early stop, at most
50 iterations, batches of 65,536 trials.  Per crossover point one child process measures both decoders
in alternation, --rounds turns each: a turn is warm-up batches, then the median of --launches batches
timed with HIP events.  The rate of a decoder is the median of its turns, its run-to-run spread the
largest minus the smallest turn; Gallager A counts as faster when the difference of the rates exceeds
five times the larger spread.  This process never opens the device: each child runs under a time limit of
its own, one at a time, and a child that fails or runs out ends the script.

  python scripts/gallager_rate.py [--out profiles/gallager_rate.json] [--scale 1]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, ITERS, ALPHA, SEED, BATCH = 10000, 50, 0.75, 11, 65536
POINTS = (0.030, 0.038)


def measure(p, args):
    """The child: both decoders at crossover probability p, in alternation; one JSON line."""
    import torch
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    torch.cuda.set_device(0)
    g = TannerGraph.random_regular(N, 3, 6, seed=1, distinct_columns=True)
    B = BATCH // args.scale
    runs = {"gallager_a": MonteCarlo(g, "bsc", p, ITERS, algo="gallager", flip_threshold=0, early_stop=True, seed=SEED,
                                     batch=B),
            "minsum": MonteCarlo(g, "bsc", p, ITERS, algo="minsum", alpha=ALPHA, early_stop=True, seed=SEED, batch=B)}
    nxt = dict.fromkeys(runs, 0)

    def batch(name):
        runs[name].run_batch(nxt[name], B)
        nxt[name] += B

    turns = {name: [] for name in runs}
    for r in range(args.rounds):
        for name in runs:
            for _ in range(args.warmup):
                batch(name)
            ms = []
            for _ in range(args.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                batch(name)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            turns[name].append(B / (statistics.median(ms) * 1e-3))
            print("p", p, "turn", r, name, "%.0f trials/s" % turns[name][-1], file=sys.stderr, flush=True)
    out = {"p": p, "batch": B, "device": torch.cuda.get_device_name(0)}
    for name, mc in runs.items():
        c = mc.counters.cpu().numpy()
        rate = statistics.median(turns[name])
        mean_its = float(c[3]) / float(c[0])
        out[name] = {"trials_per_s": rate, "turns_trials_per_s": turns[name],
                     "spread_trials_per_s": max(turns[name]) - min(turns[name]), "mean_iterations": mean_its,
                     "codeword_iterations_per_s": rate * mean_its, "trials": int(c[0]), "frame_errors": int(c[1]),
                     "bit_errors": int(c[2])}
    a, m = out["gallager_a"], out["minsum"]
    spread = max(a["spread_trials_per_s"], m["spread_trials_per_s"])
    out["gallager_a_over_minsum"] = a["trials_per_s"] / m["trials_per_s"]
    out["faster_by_more_than_5_spreads"] = bool(a["trials_per_s"] - m["trials_per_s"] > 5 * spread)
    print(json.dumps(out), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "gallager_rate.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch size (a quick run)")
    ap.add_argument("--step-seconds", type=float, default=200.0, help="time limit of one crossover point's child")
    ap.add_argument("--point", type=float, default=None, help=argparse.SUPPRESS)  # the child's mode
    args = ap.parse_args(argv)
    assert args.rounds >= 5 and args.launches >= 3
    if args.point is not None:
        return measure(args.point, args)
    out = {"n": N, "dv": 3, "dc": 6, "max_iters": ITERS, "alpha_minsum": ALPHA, "flip_threshold": 0, "seed": SEED,
           "early_stop": True, "rounds": args.rounds, "launches": args.launches, "warmup": args.warmup, "points": []}
    for p in POINTS:
        cmd = [sys.executable, os.path.abspath(__file__), "--point", repr(p), "--rounds", str(args.rounds), "--launches",
               str(args.launches), "--warmup", str(args.warmup), "--scale", str(args.scale)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.step_seconds, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("gallager_rate: p = %g ran past %g s; nothing further is started" % (p, args.step_seconds), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("gallager_rate: p = %g ended with status %d; nothing further is started" % (p, r.returncode), file=sys.stderr)
            return 1
        out["points"].append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(out["points"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
