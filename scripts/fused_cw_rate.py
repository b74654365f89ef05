"""What fusing the codeword / rate-matched Monte-Carlo of the fixed-point decoders is worth, in one
session (profiles/fused_cw_rate.json): trials/s of MonteCarlo(fused=True) against the unfused chain
(fused=False: channel entry, decode entry, count entry) of the same configuration, at three shapes --

(a) the (3,6) n = 10,000 graph of bench.py, BI-AWGN sigma = 0.85, Quant(5, 7, 2.0, 8, 1), at most 50
    iterations, early stop, random codewords, batches of 65,536;
(b) the same with one sixth of the positions punctured (scripts/rate_match_rate.py's description);
(c) qc.random_base(3, 6, 1667, seed 1) with block column 0 punctured, BSC p = 0.03, the same
    quantiser, iterations and batch (DESIGN 3.9's case (c)).

scripts/rate_match_rate.py's protocol: turns alternate between the two modes, each in a fresh child
process under a time limit of its own; a turn is a warm-up batch and the median of --launches batches
timed with HIP events; a mode's rate is the median of its --rounds turns, its spread their range.
Both modes run the same trials, so their frame and bit errors must be equal: the script ends with an
error when they are not.  This process never opens the device, and a child that fails or runs out
ends the script.

  python scripts/fused_cw_rate.py [--out profiles/fused_cw_rate.json] [--scale 1] [--shapes a,b,c]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, ITERS, BATCH, QUANT = 10000, 50, 65536, (5, 7, 2.0, 8, 1)
SHAPES = {"a": dict(code="r36_10000", channel="awgn", param=0.85, punctured="none"),
          "b": dict(code="r36_10000", channel="awgn", param=0.85, punctured="every sixth run of 1,668 positions"),
          "c": dict(code="qc.random_base(3, 6, 1667, seed=1)", channel="bsc", param=0.03, punctured="block column 0")}
MODES = ("unfused", "fused")


def turn(args):
    """A child: one turn of one mode at one shape; one JSON line."""
    import torch
    from iib_project_ldpc_codes_amd.decoder import Quant
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    torch.cuda.set_device(0)
    B = BATCH // args.scale
    shape = SHAPES[args.shape]
    if args.shape == "c":
        from iib_project_ldpc_codes_amd import qc
        code = qc.random_base(3, 6, 1667, 1)
        g, rm = code.graph(), code.rate_match(punctured_cols=[0])
    else:
        from iib_project_ldpc_codes_amd.graph import TannerGraph
        from iib_project_ldpc_codes_amd.ratematch import RateMatch
        import numpy as np
        g = TannerGraph.random_regular(N, 3, 6, seed=1, distinct_columns=True)
        # every sixth run of 1,668 positions (a multiple of four): whole groups, as a block column is
        rm = RateMatch(N, punctured=np.flatnonzero((np.arange(N) // 1668) % 6 == 0)) if args.shape == "b" else None
    mc = MonteCarlo(g, shape["channel"], shape["param"], ITERS, algo="minsum", schedule="layered", quant=Quant(*QUANT),
                    early_stop=True, seed=11, batch=B, codewords="random", rate_match=rm, fused=args.turn == "fused")
    nxt = [0]

    def batch():
        mc.run_batch(nxt[0], B)
        nxt[0] += B

    for _ in range(args.warmup):
        batch()
    ms = []
    for _ in range(args.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        batch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    c = mc.counters.cpu().numpy()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "trials_per_s": B / (statistics.median(ms) * 1e-3), "ms": ms,
                      "trials": int(c[0]), "frame_errors": int(c[1]), "bit_errors": int(c[2]),
                      "mean_iterations": float(c[3]) / float(c[0]), "channel_bit_errors": int(c[4]),
                      "n": g.n, "n_punct": 0 if rm is None else rm.n_punct}), flush=True)
    return 0


def _child(args, extra, what):
    cmd = [sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
           "--scale", str(args.scale)] + extra
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.seconds, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit("fused_cw_rate: %s ran past %g s" % (what, args.seconds))
    if r.returncode != 0:
        sys.exit("fused_cw_rate: %s ended with status %d" % (what, r.returncode))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "fused_cw_rate.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch size (a quick run)")
    ap.add_argument("--seconds", type=float, default=120.0, help="time limit of each child")
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--turn", choices=MODES, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.turn:
        return turn(args)
    out = {"max_iters": ITERS, "quant": list(QUANT), "batch": BATCH // args.scale, "rounds": args.rounds,
           "launches": args.launches, "warmup": args.warmup, "scale": args.scale, "shapes": {}}
    for s in args.shapes.split(","):
        turns = {m: [] for m in MODES}
        for r in range(args.rounds):
            for m in MODES:
                turns[m].append(_child(args, ["--turn", m, "--shape", s], "turn %d of %s at shape %s" % (r, m, s)))
                print("shape", s, "turn", r, m, "%.0f trials/s" % turns[m][-1]["trials_per_s"], file=sys.stderr, flush=True)
        rates = {}
        for m, ts in turns.items():
            v = [t["trials_per_s"] for t in ts]
            rates[m] = {"trials_per_s": statistics.median(v), "turns_trials_per_s": v, "spread_trials_per_s": max(v) - min(v),
                        **{k: ts[0][k] for k in ("trials", "frame_errors", "bit_errors", "mean_iterations",
                                                 "channel_bit_errors")}}
        u, f = rates["unfused"], rates["fused"]
        same = all(u[k] == f[k] for k in ("trials", "frame_errors", "bit_errors", "mean_iterations", "channel_bit_errors"))
        out["device"] = turns["fused"][0]["device"]
        out["shapes"][s] = dict(SHAPES[s], n=turns["fused"][0]["n"], n_punct=turns["fused"][0]["n_punct"], **rates,
                                fused_over_unfused=f["trials_per_s"] / u["trials_per_s"],
                                # positive: the fused mode is slower, in units of the unfused chain's spread
                                gap_in_unfused_spreads=(u["trials_per_s"] - f["trials_per_s"]) /
                                max(u["spread_trials_per_s"], 1e-9), counts_equal=same)
        if not same:
            print(json.dumps(out))
            sys.exit("fused_cw_rate: the two modes count differently at shape %s" % s)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:  # after every shape: a session cut short keeps what it measured
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
