"""The fixed-point layered min-sum (bp_layer_q_kernel) against the fp32 layered min-sum
(bp_layer_kernel) at the headline shape: rate, iterations and frame errors.

In one process on one device, with HIP events, on the same device-resident frames -- (3,6)
n = 10,000, B = 16,384 BI-AWGN frames at sigma = 0.85, early stop, at most 50 iterations, hard
decisions only:
  (a) --rounds alternations of [quantised, fp32]: each turn is warm-up launches, then the median
      of --launches timed ones.  The rate of a decoder is the median of its turns, its run-to-run
      spread the largest minus the smallest turn; the gain counts when the difference of the rates
      exceeds five times the larger spread;
  (b) the frame errors of both at a fixed count of 20 iterations.
Writes the numbers as JSON.

  python scripts/layered_q_rate.py [--out profiles/layered_q_rate.json] [--quant 6,8,2.0,6,0]
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
from scripts.layered_rate import ALPHA, ITERS, SEED, SIGMA, timed  # noqa: E402


def parse_quant(text):
    """bits,post_bits,scale,norm8,offset -> decoder.Quant"""
    f = text.split(",")
    if len(f) != 5:
        raise argparse.ArgumentTypeError("--quant takes bits,post_bits,scale,norm8,offset")
    try:
        return decoder.Quant(int(f[0]), int(f[1]), float(f[2]), int(f[3]), int(f[4]))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "layered_q_rate.json"))
    ap.add_argument("--quant", type=parse_quant, default=parse_quant("6,8,2.0,6,0"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch size (a quick run)")
    args = ap.parse_args(argv)
    assert args.rounds >= 5 and args.launches >= 3
    torch.cuda.set_device(0)
    g = TannerGraph.random_regular(10000, 3, 6, seed=1)
    B = 16384 // args.scale
    llr = decoder.channel_dev("awgn", SIGMA, SEED, 0, g.n, B)
    hard = torch.empty((B, g.n), dtype=torch.uint8, device="cuda")
    its = torch.empty((B,), dtype=torch.int32, device="cuda")
    layers = g.layer_schedule()
    decoders = {"quantised": args.quant, "fp32": None}

    def run(name, iters=ITERS, es=True):
        decoder.bp_decode_dev(g, llr, iters, "minsum", ALPHA, es, hard=hard, its=its, want_post=False,
                              schedule="layered", quant=decoders[name])

    out = {"device": torch.cuda.get_device_name(0), "n": g.n, "dv": 3, "dc": 6, "batch": B, "sigma": SIGMA,
           "seed": SEED, "max_iters": ITERS, "alpha_fp32": ALPHA, "quant": args.quant.as_dict(),
           "layer_rule": decoder.layer_rule(), "layers": int(layers.max()) + 1,
           "largest_layer": int(np.bincount(layers).max()), "rounds": args.rounds, "launches": args.launches,
           "warmup": args.warmup, "early_stop": {}, "fixed_20": {}}
    turns = {name: [] for name in decoders}
    stats = {}
    for r in range(args.rounds):
        for name in decoders:
            ms = statistics.median(timed(lambda: run(name), args.warmup, args.launches))
            turns[name].append(B / (ms * 1e-3))
            stats[name] = {"mean_iterations": float(its.float().mean()), "frame_errors": int(hard.any(dim=1).sum())}
            print("turn", r, name, "%.0f codewords/s" % turns[name][-1], flush=True)
    for name, rates in turns.items():
        out["early_stop"][name] = {"codewords_per_s": statistics.median(rates), "turns_codewords_per_s": rates,
                                   "spread_codewords_per_s": max(rates) - min(rates), **stats[name]}
    q, f = out["early_stop"]["quantised"], out["early_stop"]["fp32"]
    spread = max(q["spread_codewords_per_s"], f["spread_codewords_per_s"])
    out["quantised_over_fp32"] = q["codewords_per_s"] / f["codewords_per_s"]
    out["difference_over_spread"] = (q["codewords_per_s"] - f["codewords_per_s"]) / spread if spread else None
    out["faster_by_more_than_5_spreads"] = bool(q["codewords_per_s"] - f["codewords_per_s"] > 5 * spread)
    for name in decoders:
        run(name, 20, False)
        torch.cuda.synchronize()
        out["fixed_20"][name] = {"frame_errors": int(hard.any(dim=1).sum())}
    print(json.dumps({k: out[k] for k in ("early_stop", "fixed_20", "quantised_over_fp32", "difference_over_spread",
                                          "faster_by_more_than_5_spreads")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
