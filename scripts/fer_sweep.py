"""FER / BER waterfall sweeps on the device Monte-Carlo engine (configs[2] and configs[3]).

  cfg3: (3,6) n=10000, BSC, normalized min-sum, crossover sweep, ~1M trials per point
  cfg4: RSU rate-1/2 irregular (ring degree-2 placement, ensembles.py deg2="path"), n=20000,
        BI-AWGN, SPA, 100 it
  ens:  BASELINE configs[4] -- expurgated (3,6) ensemble (a fresh device-sampled graph per
        trial, parallel_simulator_expurgated.py), n=64800, BEC, 200 it, expurgation X=3;
        --channel bsc|awgn [--algo minsum|spa]: the same ensemble under soft decoding (50 it,
        early stop, no expurgation unless --expurgation is given)
  qc:   a quasi-cyclic code the user brings (--base FILE --Z Z: whitespace-separated rows of shifts,
        -1 for a zero block) or an array code (--array dv,dc,Z: shift r c mod Z, Z prime), BSC,
        min-sum, 50 it; its layers are its block rows, and --quant runs bp_qc_q_kernel
--schedule layered (cfg3, cfg4, qc): the row-serial schedule of hardware decoders on the fixed code
(decoder.bp_decode_dev; the ensemble has no layered form).
--quant bits,post_bits,scale,norm8,offset (cfg3 / qc with --schedule layered): the fixed-point layered
min-sum (decoder.Quant) -- what frame error rate a q-bit hardware decoder reaches.
--algo gallager [--flip-threshold b] (cfg3): Gallager A (b = 0) / B hard-decision decoding on the same
code and crossover points (decoder.gallager_decode_dev), to set beside min-sum.
--codewords random (cfg3, cfg4): every trial transmits a random codeword and errors are counted
against it (MonteCarlo codewords="random": encode, codeword channel, decode, count; unfused) -- no
all-zero shortcut, so a decoder's ties are not counted as correct.
--puncture / --shorten LIST (cfg3, cfg4, qc) and --puncture-cols / --shorten-cols LIST (qc: whole block
columns): rate matching (MonteCarlo rate_match=, ratematch.RateMatch) -- the listed variables are not
transmitted; a punctured one reaches the decoder as an LLR of +0, a shortened one as a known 0.  LIST:
comma-separated indices and ranges a-b, or @FILE holding them.  Errors are counted over the positions
that are not known, `rate` and `ebn0_db` are the rate-matched code's (K - n_known) / n_tx.
--fused (with --quant, and --codewords random or a rate-matching list): the two modes above in the
fixed-point decoder's own kernel (MonteCarlo fused=True) -- the same counts, and each row then carries
`error_curve`, the error rate after every iteration over the counted positions.
One process per GPU: `--gpus N` starts the N ranks itself (decided before any HIP call, refused
when fewer than N GPUs are visible -- iib_project_ldpc_codes_amd/launch.py, the same plan as
bench.py), or runs as a rank of an external torchrun; trials shard by index, counters are
all-reduced per round.  Each point stops at --stop-errors frame errors (200,
parallel_simulator.py:198), --trials, or --seconds.

  python scripts/fer_sweep.py cfg3 [--trials 1000000] [--seconds 60]
  python scripts/fer_sweep.py cfg4 --gpus 8 --seconds 300
  python scripts/fer_sweep.py ens --channel bsc --algo minsum --points 0.07,0.065
  python scripts/fer_sweep.py cfg3 --schedule layered --points 0.07
  python scripts/fer_sweep.py cfg3 --schedule layered --quant 5,7,2.0,6,0 --points 0.07
  python scripts/fer_sweep.py cfg3 --algo gallager --points 0.038,0.035,0.03
  python scripts/fer_sweep.py cfg3 --schedule layered --quant 5,7,2.0,8,1 --codewords random --points 0.06
  python scripts/fer_sweep.py qc --array 3,6,1667 --schedule layered --quant 6,8,2.0,6,0 --points 0.05
  python scripts/fer_sweep.py qc --base table.txt --Z 81 --schedule layered --points 0.04
  python scripts/fer_sweep.py qc --base table.txt --Z 81 --puncture-cols 0,1 --shorten @fill.txt --codewords random \
      --schedule layered --quant 6,8,2.0,6,0 --points 0.04
  python scripts/fer_sweep.py cfg3 --schedule layered --quant 5,7,2.0,8,1 --codewords random --fused --points 0.06
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from iib_project_ldpc_codes_amd import de, ensembles, snapshot  # noqa: E402
from iib_project_ldpc_codes_amd.launch import launch_plan, spawn_ranks  # noqa: E402
from iib_project_ldpc_codes_amd.graph import TannerGraph  # noqa: E402
from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo  # noqa: E402


def parse_quant(text):
    """bits,post_bits,scale,norm8,offset -> decoder.Quant"""
    from iib_project_ldpc_codes_amd.decoder import Quant
    f = text.split(",")
    if len(f) != 5:
        raise argparse.ArgumentTypeError("--quant takes bits,post_bits,scale,norm8,offset")
    try:
        return Quant(int(f[0]), int(f[1]), float(f[2]), int(f[3]), int(f[4]))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def parse_indices(text):
    """"3,7,10-12" or @FILE (the same, whitespace or commas between entries) -> [3, 7, 10, 11, 12]"""
    if text.startswith("@"):
        with open(text[1:]) as f:
            text = f.read()
    out = []
    try:
        for tok in text.replace(",", " ").split():
            a, _, b = tok.partition("-")
            out.extend(range(int(a), int(b) + 1) if b else [int(a)])
    except ValueError:
        raise argparse.ArgumentTypeError("an index list is comma-separated integers and ranges a-b, or @FILE")
    return out


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=["cfg3", "cfg4", "ens", "qc"])
    ap.add_argument("--base", type=str, default=None, help="qc: the base matrix file (qc.QCCode.from_text), with --Z")
    ap.add_argument("--Z", type=int, default=None, help="qc: the circulant size of --base")
    ap.add_argument("--array", type=str, default=None, metavar="DV,DC,Z", help="qc: qc.array_code(dv, dc, Z)")
    ap.add_argument("--trials", type=int, default=1_000_000)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--points", type=str, default=None)
    ap.add_argument("--checkpoint-dir", type=str, default=None,
                    help="snapshot each point there every round; a rerun resumes from it (snapshot.py)")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--stop-errors", type=int, default=200)
    ap.add_argument("--deg2", default="path", help="cfg4 degree-2 placement (ensembles.sample_irregular)")
    ap.add_argument("--expurgation", type=int, default=None,
                    help="ens: X (parallel_simulator_expurgated.py argv[9]); default 3 on the BEC, none otherwise")
    ap.add_argument("--channel", choices=["bec", "bsc", "awgn"], default="bec", help="ens: the channel")
    ap.add_argument("--algo", choices=["spa", "minsum", "gallager"], default=None,
                    help="ens on bsc / awgn: the decoder (default minsum on bsc, spa on awgn); cfg3: gallager")
    ap.add_argument("--flip-threshold", type=int, default=0,
                    help="cfg3 with --algo gallager: b (0: Gallager A, 1..14: Gallager B)")
    ap.add_argument("--schedule", choices=["flooding", "layered"], default="flooding",
                    help="cfg3 / cfg4: the decoding schedule (layered: row-serial, about half the iterations)")
    ap.add_argument("--quant", type=parse_quant, default=None, metavar="BITS,POST_BITS,SCALE,NORM8,OFFSET",
                    help="cfg3 with --schedule layered: the fixed-point layered min-sum (decoder.Quant)")
    ap.add_argument("--codewords", choices=["zero", "random"], default="zero",
                    help="cfg3 / cfg4: random transmits a random codeword per trial and counts against it "
                         "(MonteCarlo codewords=, the unfused validation mode)")
    ap.add_argument("--puncture", type=parse_indices, default=[], metavar="LIST",
                    help="cfg3 / cfg4 / qc: variables that are not transmitted (indices, ranges a-b, or @FILE)")
    ap.add_argument("--shorten", type=parse_indices, default=[], metavar="LIST",
                    help="cfg3 / cfg4 / qc: variables that are known zeros and not transmitted")
    ap.add_argument("--puncture-cols", type=parse_indices, default=[], metavar="LIST", help="qc: punctured block columns")
    ap.add_argument("--shorten-cols", type=parse_indices, default=[], metavar="LIST", help="qc: shortened block columns")
    ap.add_argument("--known-llr", type=float, default=1024.0, help="the LLR magnitude of a shortened position")
    ap.add_argument("--fused", action="store_true",
                    help="with --quant and --codewords random / a rate-matching list: channel, decode and the count of "
                         "every iteration in one kernel (MonteCarlo fused=); the rows carry error_curve")
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks, one process per GPU (default: torchrun's WORLD_SIZE, else 1); "
                         "without WORLD_SIZE the sweep starts them itself")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="allow more ranks than visible GPUs (shared devices, gloo): a rehearsal only")
    args = ap.parse_args(argv)
    if args.gpus is None:
        args.gpus = int(os.environ.get("WORLD_SIZE", "1"))
    if args.expurgation is None:
        args.expurgation = 3 if args.channel == "bec" else -1
    if args.schedule == "layered" and args.config == "ens":
        ap.error("--schedule layered needs a fixed code (cfg3, cfg4): no host-built schedule per sampled graph")
    if args.quant is not None and (args.schedule != "layered" or args.config not in ("cfg3", "qc")):
        ap.error("--quant needs cfg3 or qc (min-sum) with --schedule layered")
    if args.config == "qc":
        if (args.array is None) == (args.base is None) or (args.base is not None and args.Z is None):
            ap.error("qc needs --base FILE --Z Z, or --array dv,dc,Z")
        if args.array is not None and len(args.array.split(",")) != 3:
            ap.error("--array takes dv,dc,Z")
    elif args.base is not None or args.Z is not None or args.array is not None:
        ap.error("--base, --Z and --array belong to qc")
    if args.algo == "gallager" and (args.config != "cfg3" or args.schedule != "flooding"):
        ap.error("--algo gallager needs cfg3 with the flooding schedule (a fixed code on the BSC)")
    if args.flip_threshold and args.algo != "gallager":
        ap.error("--flip-threshold belongs to --algo gallager")
    if args.codewords == "random" and args.config == "ens":
        ap.error("--codewords random needs a fixed code (cfg3, cfg4): a per-trial graph has no encoder")
    if (args.puncture_cols or args.shorten_cols) and args.config != "qc":
        ap.error("--puncture-cols and --shorten-cols belong to qc (block columns)")
    if (args.puncture or args.shorten) and args.config == "ens":
        ap.error("--puncture and --shorten need a fixed code: a description names the variables of one graph")
    if args.fused:
        if args.quant is None:
            ap.error("--fused needs --quant (cfg3 or qc with --schedule layered): the fused codeword mode is the "
                     "fixed-point decoders'")
        if args.codewords != "random" and not (args.puncture or args.shorten or args.puncture_cols or args.shorten_cols):
            ap.error("--fused needs --codewords random or a rate-matching list: the all-zero, all-transmitted run is "
                     "fused already")
    return args


def rate_match_of(args, g):
    """The ratematch.RateMatch of the command line, or None when it names no position."""
    if not (args.puncture or args.shorten or args.puncture_cols or args.shorten_cols):
        return None
    from iib_project_ldpc_codes_amd.ratematch import RateMatch
    punct, short = list(args.puncture), list(args.shorten)
    if args.config == "qc":
        cols = g.code.rate_match(args.puncture_cols, args.shorten_cols)
        punct += [int(v) for v in cols.punctured]
        short += [int(v) for v in cols.shortened]
    return RateMatch(g.n, punct, short)


def main(argv=None):
    args = parse(argv)
    # decided before anything initialises HIP (device_count does not, on this image)
    mode, info = launch_plan(args.gpus, os.environ, torch.cuda.device_count(), args.rehearse_on_one_gpu)
    if mode == "error":
        print(f"fer_sweep: {info}", file=sys.stderr)
        return 2
    if mode == "spawn":
        return spawn_ranks(info, sys.argv[1:] if argv is None else list(argv), script=os.path.abspath(__file__))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local % max(torch.cuda.device_count(), 1))
    if world > 1:
        dist.init_process_group(os.environ.get("LDPC_DIST_BACKEND", "nccl"))
    rank = dist.get_rank() if world > 1 else 0
    if args.config == "cfg3":
        g = TannerGraph.random_regular(10000, 3, 6, seed=1, distinct_columns=True)
        channel, algo, alpha, iters = "bsc", "minsum", 0.75, 50
        points = [float(p) for p in (args.points or "0.07,0.065,0.06,0.055,0.05").split(",")]
        batch = args.batch or 65536
        if args.algo == "gallager":  # below the Gallager A threshold 0.0395 (de.gallager_threshold)
            algo = "gallager"
            points = [float(p) for p in (args.points or "0.038,0.036,0.034,0.032,0.03").split(",")]
    elif args.config == "qc":
        from iib_project_ldpc_codes_amd import qc
        code = (qc.array_code(*[int(x) for x in args.array.split(",")]) if args.array is not None
                else qc.QCCode.from_text(args.base, args.Z))
        g = code.graph()
        channel, algo, alpha, iters = "bsc", "minsum", 0.75, 50
        points = [float(p) for p in (args.points or "0.05,0.045,0.04,0.035,0.03").split(",")]
        batch = args.batch or 65536
    elif args.config == "ens":
        g = None
        channel = args.channel
        if channel == "bec":
            algo, alpha, iters, default_points = "spa", 1.0, 200, "0.425,0.42"
        else:
            algo = args.algo or ("minsum" if channel == "bsc" else "spa")
            alpha, iters = (0.75 if algo == "minsum" else 1.0), 50
            default_points = "0.07,0.065" if channel == "bsc" else "0.86,0.84"
        points = [float(p) for p in (args.points or default_points).split(",")]
        batch = args.batch or (16384 if channel == "bec" else 4096)
    else:
        g = ensembles.sample_irregular(ensembles.RSU_DL4, 20000, seed=1, deg2=args.deg2)
        channel, algo, alpha, iters = "awgn", "spa", 1.0, 100
        points = [float(p) for p in (args.points or "0.86,0.84,0.82,0.80,0.78").split(",")]
        batch = args.batch or 16384
    n, rate = (64800, 0.5) if g is None else (g.n, 1.0 - g.m / g.n)
    rm = None if g is None else rate_match_of(args, g)
    for p in points:
        if g is None:
            mc = MonteCarlo.ensemble(n, 3, 6, channel, p, iters, algo=algo, alpha=alpha, early_stop=True,
                                     expurgation=args.expurgation, seed=args.seed, batch=batch)
        else:
            mc = MonteCarlo(g, channel, p, iters, algo=algo, alpha=alpha, early_stop=True, seed=args.seed,
                            batch=batch, schedule=args.schedule, quant=args.quant, flip_threshold=args.flip_threshold,
                            codewords=args.codewords, rate_match=rm, known_llr=args.known_llr, fused=args.fused)
            if rm is not None:  # the rate-matched code's rate, from the encoder's dimension where the run has one
                K = mc.encoder.K if hasattr(mc, "encoder") else g.n - g.m
                rate = rm.rate(K)
        ck = None
        if args.checkpoint_dir:
            os.makedirs(args.checkpoint_dir, exist_ok=True)
            tag = "" if args.schedule == "flooding" else "_" + args.schedule  # flooding keeps its file names
            if args.config == "qc":  # one file per code
                tag += "_" + (args.array.replace(",", "-") if args.array is not None
                              else "%s-Z%d" % (os.path.basename(args.base), args.Z))
            if args.quant is not None:
                q = args.quant
                tag += "_q%d-%d-%g-%d-%d" % (q.bits, q.post_bits, q.scale, q.norm8, q.offset)
            if algo == "gallager":
                tag += "_gallager-b%d" % args.flip_threshold
            if args.codewords == "random":
                tag += "_cw-random"
            if rm is not None:
                tag += "_rm-" + rm.digest()[:12]
            if args.fused:
                tag += "_fused"
            ck = os.path.join(args.checkpoint_dir, f"{args.config}{tag}_p={p}_seed={args.seed}_B={batch}.json")
            if os.path.exists(ck):
                mc.restore(snapshot.load(ck))
        torch.cuda.synchronize()
        t0 = time.time()
        trials0 = int(mc.snapshot()["counters"][0])
        res = mc.run(num_tests=args.trials, stop_frame_errors=args.stop_errors, time_limit=args.seconds, checkpoint=ck)
        torch.cuda.synchronize()
        el = time.time() - t0
        if rank == 0:
            out = {"config": args.config, "expurgation": mc.expurgation, "deg2": args.deg2 if args.config == "cfg4" else None, "channel": channel, "param": p, "algo": algo, "iterations": iters,
                   "n": n, "rate": rate, "gpus": world, "trials": res["num_tests"],
                   "frame_errors": res["frame_errors"], "fer": res["fer"], "ber": res["ber"],
                   "mean_iterations": res["iterations"] / max(res["num_tests"], 1),
                   "seconds": el, "codewords_per_s": (res["num_tests"] - trials0) / el}
            if args.schedule != "flooding":
                out["schedule"] = args.schedule
            if args.config == "qc":
                out.update({"Z": g.code.Z, "base_rows": g.code.mb, "base_columns": g.code.nb})
            if args.quant is not None:
                out["quant"] = args.quant.as_dict()
            if algo == "gallager":
                out["flip_threshold"] = args.flip_threshold
            if args.codewords == "random":
                out["codewords"] = "random"
            if rm is not None:
                out["rate_match"] = dict(res["rate_match"], sha1=rm.digest(), known_llr=args.known_llr)
            if args.fused:
                out.update({"fused": True, "error_curve": [float(x) for x in res["error_curve"]]})
            if channel == "awgn":
                out["ebn0_db"] = float(de.sigma_to_ebn0_db(p, rate))
            print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
