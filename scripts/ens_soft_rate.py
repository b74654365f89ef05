"""Rate of the soft-decision ensemble Monte-Carlo against the graph sampler that feeds it.

Times, in one process on one device, with HIP events (warm-up launches, then the median of
--launches timed ones, every launch on fresh trial indices):
  * ldpc_mc_ensemble_soft_batch_dev -- BSC p = 0.07, normalized min-sum (alpha 0.75), early stop,
    50 iterations -- at (3,6) n = 10,000 (B = 16,384) and n = 64,800 (B = 4,096);
  * ldpc_sample_regular_dev alone on the same (n, B);
  * the BEC ensemble batch (ldpc_mc_ensemble_batch_dev, eps = 0.427, 200 iterations, X = 3) at
    n = 64,800, the existing yardstick.
Writes trials/s, graphs/s and the decode share 1 - t_sampler / t_total as JSON.

  python scripts/ens_soft_rate.py [--out profiles/ens_soft_rate.json] [--launches 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from iib_project_ldpc_codes_amd import _native  # noqa: E402

SEED, P, ITERS, ALPHA = 11, 0.07, 50, 0.75
SHAPES = [(10000, 16384), (64800, 4096)]


def timed(launch, warmup, launches):
    """Milliseconds of launch(i), i = 0 .. : warm-up launches untimed, then one event pair each."""
    for i in range(warmup):
        launch(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(warmup, warmup + launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        launch(i)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms


def summary(ms, B):
    med = statistics.median(ms)
    return {"launch_ms_median": med, "launch_ms_min": min(ms), "launch_ms_max": max(ms), "launches": len(ms),
            "per_s": B / (med * 1e-3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "ens_soft_rate.json"))
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch sizes (a quick run, e.g. under a profiler)")
    ap.add_argument("--only-n", type=int, default=0, help="time this block length only")
    args = ap.parse_args(argv)
    assert args.launches >= 5
    L = _native.lib()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"device": torch.cuda.get_device_name(0), "channel": "bsc", "param": P, "algo": "minsum", "alpha": ALPHA,
           "early_stop": True, "iterations": ITERS, "seed": SEED, "shapes": []}
    for n, B in SHAPES:
        if args.only_n and n != args.only_n:
            continue
        B //= args.scale
        E = 3 * n
        counters = torch.zeros(_native.MC_NCOUNT + ITERS + 1, dtype=torch.int64, device="cuda")

        def soft(i):
            _native.check(L.ldpc_mc_ensemble_soft_batch_dev(n, 3, 6, _native.CH_BSC, P, _native.ALGO_MINSUM, ALPHA, 1,
                                                            SEED, i * B, B, ITERS, -1, 0, counters.data_ptr(), stream),
                          "ldpc_mc_ensemble_soft_batch_dev")

        ms_soft = timed(soft, args.warmup, args.launches)
        c = counters.cpu().numpy()
        chk = torch.empty((B, E), dtype=torch.int32, device="cuda")
        var = torch.empty((B, E), dtype=torch.int32, device="cuda")

        def sample(i):
            _native.check(L.ldpc_sample_regular_dev(n, 3, 6, SEED, i * B, B, chk.data_ptr(), var.data_ptr(), None,
                                                    stream), "ldpc_sample_regular_dev")

        ms_samp = timed(sample, args.warmup, args.launches)
        del chk, var
        row = {"n": n, "dv": 3, "dc": 6, "batch": B, "soft": summary(ms_soft, B), "sampler": summary(ms_samp, B),
               "trials": int(c[0]), "fer": float(c[1] / c[0]), "mean_iterations": float(c[3] / c[0])}
        row["trials_per_s"] = row["soft"]["per_s"]
        row["graphs_per_s"] = row["sampler"]["per_s"]
        row["decode_share"] = 1.0 - row["sampler"]["launch_ms_median"] / row["soft"]["launch_ms_median"]
        if n == 64800:
            cb = torch.zeros(_native.MC_NCOUNT + 200 + 1, dtype=torch.int64, device="cuda")

            def bec(i):
                _native.check(L.ldpc_mc_ensemble_batch_dev(n, 3, 6, _native.CH_BEC, 0.427, SEED, i * B, B, 200, 3, 0,
                                                           cb.data_ptr(), stream), "ldpc_mc_ensemble_batch_dev")

            row["bec_ensemble"] = summary(timed(bec, args.warmup, args.launches), B)
            row["bec_ensemble"]["decode_share"] = 1.0 - (row["sampler"]["launch_ms_median"] /
                                                         row["bec_ensemble"]["launch_ms_median"])
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
