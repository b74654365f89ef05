"""bench.py --dump-outputs on the GPU: a plain run (no --full) of the headline step on a small
batch writes post / hard / its of its last timed step as float32 .npy files, and they equal what
the same decode gives in this process on the same seeded inputs, value for value (the kernel is
deterministic and the inputs depend only on the arguments).  The line of such a run carries no
extras and no CPU baseline, and `steps` / `ms_per_step` are those of the timed loop."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_step_outputs(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import bench
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    B = 96  # fewer frames than bench.DUMP_FRAMES: every frame is dumped, in order
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(B), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if k != "WORLD_SIZE"})
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["extras"] == {} and line["cpu_baseline"] is None
    assert sorted(os.listdir(out)) == ["hard.npy", "its.npy", "post.npy"]
    got = {k: np.load(out / (k + ".npy")) for k in ("post", "hard", "its")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64e6

    g = TannerGraph.random_regular(bench.N_BITS, bench.DV, bench.DC, seed=1)
    llr = decoder.channel_dev("awgn", bench.SIGMA, 2026, 0, g.n, B)
    post, hard, its = decoder.bp_decode_dev(g, llr, bench.ITERS, "spa", early_stop=False)
    torch.cuda.synchronize()
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(B, size=min(bench.DUMP_FRAMES, B), replace=False))
    assert np.array_equal(rows, np.arange(B))
    assert got["post"].shape == (B, g.n) and np.array_equal(got["post"], post.cpu().numpy()[rows])
    assert np.array_equal(got["hard"], hard.cpu().numpy()[rows].astype(np.float32))
    assert np.array_equal(got["its"], np.full(B, bench.ITERS, np.float32))
    assert np.array_equal(got["its"], its.cpu().numpy().astype(np.float32))
