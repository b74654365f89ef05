"""What rate matching costs and what a rate-matched quasi-cyclic run shows, in one session
(profiles/rate_match_rate.json):

(a) trials/s of MonteCarlo(rate_match=all-transmitted, codewords="random") against
    MonteCarlo(codewords="random") at the configs[2] shape of bench.py (BSC p = 0.07, min-sum
    alpha = 0.75, at most 50 iterations, early stop, batches of 65,536): the same chain plus one
    description byte per variable;
(b) the same with one sixth of the positions punctured in whole groups of four (every sixth run of
    1,668 variables, which is what a punctured block column is): the path that draws nothing.  BSC
    p = 0.07 is beyond that code's threshold, so its Monte-Carlo rate is that of 50 iterations on every
    trial; each turn therefore also times the channel entry alone (median of five launches);
(c) frame errors and mean iterations of a rate-matched quasi-cyclic run, qc.random_base(3, 6, 1667,
    seed 1) with block column 0 punctured, random codewords, BSC p = 0.03, 16,384 trials, for both
    Quant sets of DESIGN section 7.

Turns alternate, each in a fresh child process under a time limit of its own: a turn is a warm-up
batch and the median of --launches batches timed with HIP events; a mode's rate is the median of its
--rounds turns, its spread their range.  This process never opens the device, and a child that fails
or runs out ends the script.

  python scripts/rate_match_rate.py [--out profiles/rate_match_rate.json] [--scale 1]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, ITERS, ALPHA, BATCH, P = 10000, 50, 0.75, 65536, 0.07
MODES = ("codewords_random", "rate_match_all_tx", "rate_match_sixth_punctured")
QUANTS = {"layered_q_6_8_2.0_6_0": (6, 8, 2.0, 6, 0), "layered_q_5_7_2.0_8_1": (5, 7, 2.0, 8, 1)}
QC = dict(mb=3, nb=6, Z=1667, seed=1, punctured_cols=[0], p=0.03, trials=16384)


def _sixth(n):
    """Every sixth run of 1,668 positions (a multiple of four): whole groups, as a block column is."""
    import numpy as np
    run = 1668
    return np.flatnonzero((np.arange(n) // run) % 6 == 0)


def turn(args):
    """A child: one mode's turn; one JSON line."""
    import torch
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    from iib_project_ldpc_codes_amd.ratematch import RateMatch
    torch.cuda.set_device(0)
    B = BATCH // args.scale
    g = TannerGraph.random_regular(N, 3, 6, seed=1, distinct_columns=True)
    rm = {"codewords_random": None, "rate_match_all_tx": RateMatch(N),
          "rate_match_sixth_punctured": RateMatch(N, punctured=_sixth(N))}[args.turn]
    mc = MonteCarlo(g, "bsc", P, ITERS, algo="minsum", alpha=ALPHA, early_stop=True, seed=11, batch=B,
                    codewords="random", rate_match=rm)
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
    # the channel entry of the mode alone, on the batch's own codewords: where the skipped draws show
    from iib_project_ldpc_codes_amd import decoder
    cw = mc.encoder.random_codewords_dev(11, 0, B)[0]
    llr = torch.empty((B, N), dtype=torch.float32, device="cuda")
    chan = []
    for i in range(args.warmup + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        decoder.channel_dev("bsc", P, 11, 0, N, B, out=llr, codewords=cw, rate_match=rm)
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            chan.append(e0.elapsed_time(e1))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "trials_per_s": B / (statistics.median(ms) * 1e-3),
                      "channel_ms": statistics.median(chan), "ms": ms, "trials": int(c[0]), "frame_errors": int(c[1]), "bit_errors": int(c[2]),
                      "mean_iterations": float(c[3]) / float(c[0]), "n_punct": 0 if rm is None else rm.n_punct}), flush=True)
    return 0


def qc_run(args):
    """A child: part (c); one JSON line."""
    import torch
    from iib_project_ldpc_codes_amd import qc
    from iib_project_ldpc_codes_amd.decoder import Quant
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    torch.cuda.set_device(0)
    code = qc.random_base(QC["mb"], QC["nb"], QC["Z"], QC["seed"])
    g = code.graph()
    rm = code.rate_match(punctured_cols=QC["punctured_cols"])
    T = QC["trials"] // args.scale
    out = {}
    for name, q in QUANTS.items():
        mc = MonteCarlo(g, "bsc", QC["p"], ITERS, algo="minsum", schedule="layered", quant=Quant(*q), early_stop=True,
                        seed=2026, batch=T, codewords="random", rate_match=rm)
        mc.run_batch(0, T)
        c = mc.counters.cpu().numpy()
        assert int(c[0]) == T
        out[name] = {"trials": T, "frame_errors": int(c[1]), "bit_errors": int(c[2]), "mean_iterations": float(c[3]) / T,
                     "channel_bit_errors": int(c[4])}
    print(json.dumps({"n": g.n, "K": mc.encoder.K, "n_tx": rm.n_tx, "n_punct": rm.n_punct, "rate": rm.rate(mc.encoder.K),
                      "runs": out}), flush=True)
    return 0


def _child(args, extra, what):
    cmd = [sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
           "--scale", str(args.scale)] + extra
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.seconds, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit("rate_match_rate: %s ran past %g s" % (what, args.seconds))
    if r.returncode != 0:
        sys.exit("rate_match_rate: %s ended with status %d" % (what, r.returncode))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "rate_match_rate.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch sizes (a quick run)")
    ap.add_argument("--seconds", type=float, default=120.0, help="time limit of each child")
    ap.add_argument("--turn", choices=MODES, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--qc", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.turn:
        return turn(args)
    if args.qc:
        return qc_run(args)
    turns = {m: [] for m in MODES}
    for r in range(args.rounds):
        for m in MODES:
            turns[m].append(_child(args, ["--turn", m], "turn %d of %s" % (r, m)))
            print("turn", r, m, "%.0f trials/s" % turns[m][-1]["trials_per_s"], file=sys.stderr, flush=True)
    rates = {}
    for m, ts in turns.items():
        v = [t["trials_per_s"] for t in ts]
        rates[m] = {"trials_per_s": statistics.median(v), "turns_trials_per_s": v, "spread_trials_per_s": max(v) - min(v),
                    "channel_ms": statistics.median(t["channel_ms"] for t in ts),
                    "turns_channel_ms": [t["channel_ms"] for t in ts], "n_punct": ts[0]["n_punct"], "trials": ts[0]["trials"], "frame_errors": ts[0]["frame_errors"],
                    "bit_errors": ts[0]["bit_errors"], "mean_iterations": ts[0]["mean_iterations"]}
    base = rates["codewords_random"]
    for m in MODES[1:]:
        rates[m]["over_codewords_random"] = rates[m]["trials_per_s"] / base["trials_per_s"]
        rates[m]["gap_in_spreads"] = ((base["trials_per_s"] - rates[m]["trials_per_s"]) /
                                      max(base["spread_trials_per_s"], rates[m]["spread_trials_per_s"], 1e-9))
    out = {"n": N, "dv": 3, "dc": 6, "channel": "bsc", "param": P, "max_iters": ITERS, "alpha": ALPHA,
           "batch": BATCH // args.scale, "rounds": args.rounds, "launches": args.launches, "warmup": args.warmup,
           "scale": args.scale, "device": turns[MODES[0]][0]["device"], "mc_rate_cfg2_p0.07": rates,
           "qc_rate_matched": dict(QC, **_child(args, ["--qc"], "the quasi-cyclic run"))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
