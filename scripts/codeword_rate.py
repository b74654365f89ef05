"""What the codeword family costs and what it shows, in one session (profiles/codeword_rate.json):

(a) ldpc_encoder_create seconds (host elimination + upload) at (3,6) n = 10,000 and at the n = 20,000
    ring code (scripts/fer_sweep.py cfg4), and the encode of 65,536 codewords at n = 10,000 beside the
    fixed-count (50 iterations) min-sum decode of the same batch;
(b) trials/s of MonteCarlo(codewords="random") against the fused all-zero Monte-Carlo at the
    configs[2] shape of bench.py (BSC p = 0.07, min-sum alpha = 0.75, at most 50 iterations, early stop,
    batches of 65,536), in alternation: --rounds turns each, a turn is a warm-up batch and the median of
    --launches batches timed with HIP events; the rate is the median of the turns;
(c) frame errors of 16,384 trials in both modes at the shapes of profiles/layered_q_rate.json and
    profiles/layered_q_rate_offset.json ((3,6) n = 10,000 seed 1, BI-AWGN sigma = 0.85, at most 50
    iterations, early stop, seed 2026), for fp32 layered min-sum there too, and for Gallager A at
    p = 0.038 on the cfg3 code.

This process never opens the device: one child does the measuring under a time limit of its own, and
a child that fails or runs out ends the script.

  python scripts/codeword_rate.py [--out profiles/codeword_rate.json] [--scale 1]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, ITERS, ALPHA, BATCH = 10000, 50, 0.75, 65536
QUANTS = {"layered_q_6_8_2.0_6_0": (6, 8, 2.0, 6, 0), "layered_q_5_7_2.0_8_1": (5, 7, 2.0, 8, 1)}


def _median_ms(torch, fn, warmup, launches):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def measure(args):
    """The child: the three parts; one JSON line."""
    import torch
    from iib_project_ldpc_codes_amd import decoder, ensembles
    from iib_project_ldpc_codes_amd.decoder import Quant
    from iib_project_ldpc_codes_amd.encoder import Encoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0)}
    say = lambda *a: print(*a, file=sys.stderr, flush=True)  # noqa: E731

    # ---- (a) encoder build and encode time
    g = TannerGraph.random_regular(N, 3, 6, seed=1)
    ring = ensembles.sample_irregular(ensembles.RSU_DL4, 20000, seed=1, deg2="path")
    build = {}
    for name, gr in (("r36_10000", g), ("rsu_ring_20000", ring)):
        gr.handle()
        t0 = time.perf_counter()
        enc = Encoder(gr)
        build[name] = {"n": gr.n, "m": gr.m, "rank": enc.rank, "K": enc.K, "create_seconds": time.perf_counter() - t0}
        say("create", name, build[name])
        if gr is g:
            enc10k = enc
    B = BATCH // args.scale
    info = enc10k.info_bits_dev(1, 0, B)
    cw = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    enc_ms, enc_all = _median_ms(torch, lambda: enc10k.encode_dev(info, out=cw), 2, 5)
    llr = decoder.channel_dev("bsc", 0.07, 1, 0, N, B, codewords=cw)
    hard = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    its = torch.empty((B,), dtype=torch.int32, device="cuda")
    dec_ms, dec_all = _median_ms(torch, lambda: decoder.bp_decode_dev(g, llr, ITERS, "minsum", ALPHA, False, hard=hard,
                                                                       its=its, want_post=False), 2, 5)
    chan_ms, _ = _median_ms(torch, lambda: decoder.channel_dev("bsc", 0.07, 1, 0, N, B, out=llr, codewords=cw), 2, 5)
    info_ms, _ = _median_ms(torch, lambda: enc10k.info_bits_dev(1, 0, B, out=info), 2, 5)
    out["encoder"] = {"build": build, "batch": B, "encode_ms": enc_ms, "encode_ms_all": enc_all,
                      "minsum_fixed_%d_decode_ms" % ITERS: dec_ms, "decode_ms_all": dec_all,
                      "encode_over_decode": enc_ms / dec_ms, "codeword_channel_ms": chan_ms, "info_bits_ms": info_ms,
                      "word_ops": enc10k.rank * enc10k.K * (B // 32)}
    say("encode", out["encoder"])
    del llr, hard, cw, info

    # ---- (b) Monte-Carlo rates at the configs[2] shape
    gd = TannerGraph.random_regular(N, 3, 6, seed=1, distinct_columns=True)
    runs = {mode: MonteCarlo(gd, "bsc", 0.07, ITERS, algo="minsum", alpha=ALPHA, early_stop=True, seed=11, batch=B,
                             codewords=mode) for mode in ("zero", "random")}
    nxt = dict.fromkeys(runs, 0)

    def batch(mode):
        runs[mode].run_batch(nxt[mode], B)
        nxt[mode] += B

    turns = {mode: [] for mode in runs}
    for r in range(args.rounds):
        for mode in runs:
            ms, _ = _median_ms(torch, lambda: batch(mode), args.warmup, args.launches)
            turns[mode].append(B / (ms * 1e-3))
            say("turn", r, mode, "%.0f trials/s" % turns[mode][-1])
    rates = {}
    for mode, mc in runs.items():
        c = mc.counters.cpu().numpy()
        rates[mode] = {"trials_per_s": statistics.median(turns[mode]), "turns_trials_per_s": turns[mode],
                       "spread_trials_per_s": max(turns[mode]) - min(turns[mode]), "trials": int(c[0]),
                       "frame_errors": int(c[1]), "bit_errors": int(c[2]), "mean_iterations": float(c[3]) / float(c[0])}
    rates["random_over_zero"] = rates["random"]["trials_per_s"] / rates["zero"]["trials_per_s"]
    out["mc_rate_cfg2_p0.07"] = rates
    del runs

    # ---- (c) frame errors of 16,384 trials in both modes
    T = 16384 // args.scale
    fe = {}
    cases = [(name, g, "awgn", 0.85, 2026, dict(algo="minsum", schedule="layered", quant=Quant(*q)))
             for name, q in QUANTS.items()]
    cases.append(("layered_fp32_minsum_0.75", g, "awgn", 0.85, 2026, dict(algo="minsum", alpha=ALPHA, schedule="layered")))
    cases.append(("gallager_a_p0.038", gd, "bsc", 0.038, 11, dict(algo="gallager")))
    for name, gr, ch, p, seed, kw in cases:
        row = {"channel": ch, "param": p, "seed": seed, "trials": T}
        for mode in ("zero", "random"):
            mc = MonteCarlo(gr, ch, p, ITERS, early_stop=True, seed=seed, batch=T, codewords=mode, **kw)
            mc.run_batch(0, T)
            c = mc.counters.cpu().numpy()
            assert int(c[0]) == T
            row[mode] = {"frame_errors": int(c[1]), "bit_errors": int(c[2]), "mean_iterations": float(c[3]) / T,
                         "channel_bit_errors": int(c[4])}
        fe[name] = row
        say("frame errors", name, row)
    out["frame_errors_16384"] = fe
    print(json.dumps(out), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "codeword_rate.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch sizes (a quick run)")
    ap.add_argument("--seconds", type=float, default=420.0, help="time limit of the measuring child")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.child:
        return measure(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds), "--launches",
           str(args.launches), "--warmup", str(args.warmup), "--scale", str(args.scale)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.seconds, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print("codeword_rate: the child ran past %g s" % args.seconds, file=sys.stderr)
        return 1
    if r.returncode != 0:
        print("codeword_rate: the child ended with status %d" % r.returncode, file=sys.stderr)
        return 1
    out = {"n": N, "dv": 3, "dc": 6, "max_iters": ITERS, "alpha": ALPHA, "rounds": args.rounds, "launches": args.launches,
           "warmup": args.warmup, "scale": args.scale}
    out.update(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
