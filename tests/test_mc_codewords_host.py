"""The codewords argument of MonteCarlo without a device: which configurations it refuses, what a
snapshot records, which resumes are refused, and that an all-zero run's snapshot is byte for byte
what it was (the batches run on a stand-in executor, as tests/test_layer_q_snapshot.py's)."""
import json

import numpy as np
import pytest

from iib_project_ldpc_codes_amd import snapshot
from iib_project_ldpc_codes_amd.decoder import Quant
from iib_project_ldpc_codes_amd.graph import TannerGraph
from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo

B, ITERS = 32, 10


def _executor(first_cw, batch, stop_frame_errors, counters, stream=None):
    counters[0] += batch
    counters[1] += 1
    counters[2] += 7
    counters[4] += 40        # curve[0]: channel errors
    counters[4 + ITERS] += 7  # curve[max_iters]: final errors


def _graph():
    return TannerGraph.random_regular(120, 3, 6, seed=1)


def _mc(**kw):
    kw.setdefault("algo", "minsum")
    return MonteCarlo(_graph(), kw.pop("channel", "bsc"), kw.pop("param", 0.07), ITERS, alpha=0.75, seed=5, batch=B,
                      executor=_executor, **kw)


def test_argument_errors():
    for kw in (dict(channel="bec", param=0.4, algo="spa"),   # erasure decoding does not depend on the codeword
               dict(channel="bec", param=0.4, algo="spa", optimal=True),  # the ML modes
               dict(codewords="one"), dict(codewords=None), dict(codewords=True)):
        kw.setdefault("codewords", "random")
        with pytest.raises(ValueError):
            _mc(**kw)
    with pytest.raises(ValueError):  # a per-trial graph has no encoder
        MonteCarlo.ensemble(120, 3, 6, "bsc", 0.07, ITERS, algo="minsum", executor=_executor, codewords="random")
    # every fixed-code decoder on the BSC / BI-AWGN takes the mode
    for kw in (dict(), dict(algo="spa"), dict(channel="awgn", param=0.8), dict(schedule="layered"),
               dict(schedule="layered", quant=Quant(6, 8, 2.0)), dict(algo="gallager"),
               dict(algo="gallager", flip_threshold=2)):
        assert _mc(codewords="random", **kw).codewords == "random"
    assert _mc().codewords == "zero" and _mc(codewords="zero").codewords == "zero"


def test_only_a_random_run_records_the_mode():
    for kw in (dict(), dict(schedule="layered"), dict(algo="gallager")):
        zero, rnd = snapshot.config(_mc(**kw)), snapshot.config(_mc(codewords="random", **kw))
        assert "codewords" not in zero and zero == snapshot.config(_mc(codewords="zero", **kw))
        assert rnd["codewords"] == "random"
        assert {k: v for k, v in rnd.items() if k != "codewords"} == zero


def test_zero_snapshot_bytes_unchanged(tmp_path):
    """The file of an all-zero run, key for key and byte for byte as it was before the mode existed."""
    a = _mc()
    a.run(2 * B, stop_frame_errors=0)
    path = str(tmp_path / "zero.json")
    snapshot.save(a.snapshot(), path)
    g = _graph()
    want = {"version": 1,
            "config": {"graph": snapshot.graph_fingerprint(g), "channel": 1, "param": 0.07, "max_iters": ITERS,
                       "algo": 1, "alpha": 0.75, "early_stop": True, "expurgation": -1, "optimal": False,
                       "message_passing": True},
            "seed": 5, "trial_ranges": [[0, 2 * B]],
            "counters": [2 * B, 2, 14, 0, 80] + [0] * (ITERS - 1) + [14], "counters_ml": None}
    with open(path) as f:
        assert f.read() == json.dumps(want)
    b = _mc(codewords="zero")
    b.run(2 * B, stop_frame_errors=0)
    assert json.dumps(b.snapshot()) == json.dumps(want)


def test_resume_within_a_mode_only(tmp_path):
    a = _mc(codewords="random")
    a.run(2 * B, stop_frame_errors=0)
    path = str(tmp_path / "random.json")
    snapshot.save(a.snapshot(), path)
    assert snapshot.load(path)["config"]["codewords"] == "random"
    b = _mc(codewords="random")
    b.restore(snapshot.load(path))
    assert b.next_trial() == 2 * B and int(b.counters[0]) == 2 * B
    with pytest.raises(ValueError):
        _mc().restore(snapshot.load(path))
    zero = _mc()
    zero.run(B, stop_frame_errors=0)
    with pytest.raises(ValueError):
        _mc(codewords="random").restore(zero.snapshot())
    with pytest.raises(ValueError):
        snapshot.merge([a.snapshot(), zero.snapshot()])


def test_results_report_the_two_ends():
    a = _mc(codewords="random")
    r = a.run(2 * B, stop_frame_errors=0)
    assert r["codewords"] == "random" and r["channel_bit_errors"] == 80 and r["bit_errors"] == 14
    curve = r["error_curve"]
    assert curve[0] == 80 / (120 * 2 * B) and curve[-1] == 14 / (120 * 2 * B) and np.isnan(curve[1:-1]).all()
    z = _mc().run(2 * B, stop_frame_errors=0)
    assert "codewords" not in z and not np.isnan(z["error_curve"]).any()


def test_fer_sweep_takes_the_mode():
    from tests.test_fer_sweep_launch import _load
    fs = _load()
    assert fs.parse(["cfg3"]).codewords == "zero"
    assert fs.parse(["cfg3", "--schedule", "layered", "--quant", "5,7,2.0,8,1", "--codewords", "random"]).codewords == "random"
    assert fs.parse(["cfg4", "--codewords", "random"]).codewords == "random"
    with pytest.raises(SystemExit):  # a per-trial graph has no encoder
        fs.parse(["ens", "--codewords", "random"])
