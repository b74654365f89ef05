"""The quasi-cyclic fixed-point layered min-sum (bp_qc_q_kernel) against bp_layer_q_kernel: rate,
iterations and frame errors at the headline shape.

B = 16,384 BI-AWGN frames at sigma = 0.85, early stop, at most 50 iterations, hard decisions only,
the two parameter sets of scripts/layered_q_rate.py, three decoders:
  qc      bp_qc_q_kernel on qc.array_code(3, 6, 1667), n = 10,002, three block-row layers;
  table   bp_layer_q_kernel on the same graph and block-row schedule (LDPC_NO_QC_KERNEL=1);
  random  bp_layer_q_kernel on the random (3,6) n = 10,000 graph under the colouring (nine layers):
          the figures of profiles/layered_q_rate*.json.
--rounds alternations of [qc, table, random]; every turn is a fresh child process of this script
(--turn NAME: warm-up launches, then the median of --launches timed ones, per parameter set) under
its own time limit, and the first turn that fails ends the run.  The rate of a decoder is the median
of its turns, its run-to-run spread the largest minus the smallest turn.  qc counts as faster than
table when the difference of the rates exceeds five times table's spread; their frame errors and
mean iterations must be equal (same arithmetic, same schedule).  random is another code and
schedule: reported, not compared.  Writes the numbers as JSON.

  python scripts/qc_rate.py [--out profiles/qc_rate.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = ["6,8,2.0,6,0", "5,7,2.0,8,1"]
DECODERS = ("qc", "table", "random")
TURN_LIMIT_S = 240


def turn(name, args):
    """One turn of one decoder in this process: a JSON line {set: {rate, iterations, frame errors}}."""
    import torch

    from iib_project_ldpc_codes_amd import decoder, qc
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from scripts.layered_q_rate import parse_quant
    from scripts.layered_rate import ITERS, SEED, SIGMA, timed
    torch.cuda.set_device(0)
    assert (os.environ.get("LDPC_NO_QC_KERNEL") == "1") == (name == "table")
    g = TannerGraph.random_regular(10000, 3, 6, seed=1) if name == "random" else qc.array_code(3, 6, 1667).graph()
    B = 16384 // args.scale
    llr = decoder.channel_dev("awgn", SIGMA, SEED, 0, g.n, B)
    hard = torch.empty((B, g.n), dtype=torch.uint8, device="cuda")
    its = torch.empty((B,), dtype=torch.int32, device="cuda")
    layers = g.layer_schedule()
    out = {"n": g.n, "layer_rule": decoder.layer_rule(g), "layers": int(layers.max()) + 1, "sets": {}}
    for text in SETS:
        q = parse_quant(text)

        def run():
            decoder.bp_decode_dev(g, llr, ITERS, "minsum", 1.0, True, hard=hard, its=its, want_post=False,
                                  schedule="layered", quant=q)
        ms = statistics.median(timed(run, args.warmup, args.launches))
        out["sets"][text] = {"codewords_per_s": B / (ms * 1e-3), "mean_iterations": float(its.float().mean()),
                             "frame_errors": int(hard.any(dim=1).sum())}
    print("TURN " + json.dumps(out), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "qc_rate.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch size (a quick run)")
    ap.add_argument("--turn", choices=DECODERS, default=None, help="one turn of one decoder in this process")
    args = ap.parse_args(argv)
    assert args.rounds >= 5 and args.launches >= 3
    if args.turn:
        return turn(args.turn, args)
    turns = {name: [] for name in DECODERS}
    for r in range(args.rounds):
        for name in DECODERS:
            env = {k: v for k, v in os.environ.items() if k != "LDPC_NO_QC_KERNEL"}
            if name == "table":
                env["LDPC_NO_QC_KERNEL"] = "1"
            cmd = [sys.executable, os.path.abspath(__file__), "--turn", name, "--launches", str(args.launches),
                   "--warmup", str(args.warmup), "--scale", str(args.scale)]
            try:
                p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, universal_newlines=True,
                                   timeout=TURN_LIMIT_S)
            except subprocess.TimeoutExpired:
                print("turn", r, name, "ran into its time limit: nothing more is started", flush=True)
                return 1
            if p.returncode != 0:
                print("turn", r, name, "failed with status", p.returncode, ": nothing more is started", flush=True)
                return 1
            line = [x for x in p.stdout.splitlines() if x.startswith("TURN ")][-1]
            turns[name].append(json.loads(line[5:]))
            print("turn", r, name, " ".join("%.0f" % s["codewords_per_s"] for s in turns[name][-1]["sets"].values()),
                  "codewords/s", flush=True)
    out = {"batch": 16384 // args.scale, "sigma": 0.85, "max_iters": 50, "rounds": args.rounds,
           "launches": args.launches, "warmup": args.warmup, "sets": {}}
    ok = True
    for text in SETS:
        res = {}
        for name in DECODERS:
            rates = [t["sets"][text]["codewords_per_s"] for t in turns[name]]
            last = turns[name][-1]
            res[name] = {"n": last["n"], "layer_rule": last["layer_rule"], "layers": last["layers"],
                         "codewords_per_s": statistics.median(rates), "turns_codewords_per_s": rates,
                         "spread_codewords_per_s": max(rates) - min(rates),
                         "mean_iterations": last["sets"][text]["mean_iterations"],
                         "frame_errors": last["sets"][text]["frame_errors"]}
        a, b, c = res["qc"], res["table"], res["random"]
        res["qc_equals_table"] = bool(a["frame_errors"] == b["frame_errors"] and
                                      a["mean_iterations"] == b["mean_iterations"])
        ok &= res["qc_equals_table"]
        diff = a["codewords_per_s"] - b["codewords_per_s"]
        res["qc_over_table"] = a["codewords_per_s"] / b["codewords_per_s"]
        res["difference_over_table_spread"] = diff / b["spread_codewords_per_s"] if b["spread_codewords_per_s"] else None
        res["qc_faster_by_more_than_5_spreads"] = bool(diff > 5 * b["spread_codewords_per_s"])
        res["table_over_random"] = b["codewords_per_s"] / c["codewords_per_s"]  # three layers instead of nine
        out["sets"][text] = res
    print(json.dumps({k: {x: v[x] for x in ("qc_over_table", "difference_over_table_spread",
                                            "qc_faster_by_more_than_5_spreads", "table_over_random", "qc_equals_table")}
                      for k, v in out["sets"].items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    if not ok:
        print("frame errors or mean iterations of qc and table differ", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
