"""The schedule argument of the Python layer, without a device: what MonteCarlo accepts, what a
snapshot records, which resumes are refused (the batches run on a stand-in executor, as
tests/test_snapshot.py's)."""
import numpy as np
import pytest

from iib_project_ldpc_codes_amd import snapshot
from iib_project_ldpc_codes_amd.graph import TannerGraph
from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo

B, ITERS = 32, 10


def _executor(first_cw, batch, stop_frame_errors, counters, stream=None):
    counters[0] += batch
    counters[1] += 1


def _mc(schedule=None, channel="bsc", **kw):
    g = TannerGraph.random_regular(120, 3, 6, seed=1)
    extra = {} if schedule is None else {"schedule": schedule}
    return MonteCarlo(g, channel, 0.07, ITERS, algo="minsum", alpha=0.75, seed=5, batch=B, executor=_executor,
                      **extra, **kw)


def test_flooding_config_is_what_it_was():
    """No new field for flooding runs: their snapshots stay byte for byte, and merge with old ones."""
    assert snapshot.config(_mc()) == snapshot.config(_mc("flooding"))
    assert "schedule" not in snapshot.config(_mc()) and "layer_rule" not in snapshot.config(_mc())
    cfg = snapshot.config(_mc("layered"))
    assert cfg["schedule"] == "layered" and cfg["layer_rule"] == snapshot.LAYER_RULE
    assert {k: v for k, v in cfg.items() if k not in ("schedule", "layer_rule")} == snapshot.config(_mc())


def test_resume_within_a_schedule_and_refusal_across(tmp_path):
    for sched in ("flooding", "layered"):
        a = _mc(sched)
        a.run(2 * B, stop_frame_errors=0)
        path = str(tmp_path / (sched + ".json"))
        snapshot.save(a.snapshot(), path)
        b = _mc(sched)
        b.restore(snapshot.load(path))
        assert b.next_trial() == 2 * B and int(b.counters[0]) == 2 * B
        other = _mc("layered" if sched == "flooding" else "flooding")
        with pytest.raises(ValueError):
            other.restore(snapshot.load(path))
    # a snapshot written before the field existed is a flooding run
    old = snapshot.load(str(tmp_path / "flooding.json"))
    assert "schedule" not in old["config"]
    _mc().restore(old)
    with pytest.raises(ValueError):
        _mc("layered").restore(old)
    # a layered snapshot of another colouring rule does not resume
    lay = snapshot.load(str(tmp_path / "layered.json"))
    lay["config"]["layer_rule"] = "first-fit/check-order/v0"
    with pytest.raises(ValueError):
        _mc("layered").restore(lay)


def test_what_the_layered_schedule_does_not_cover():
    with pytest.raises(ValueError):
        MonteCarlo.ensemble(1200, 3, 6, "bsc", 0.07, ITERS, executor=_executor, schedule="layered")
    with pytest.raises(ValueError):
        _mc("layered", channel="bec")
    with pytest.raises(ValueError):
        _mc("serial")
    MonteCarlo.ensemble(1200, 3, 6, "bsc", 0.07, ITERS, executor=_executor, schedule="flooding")


def test_layer_schedule_method_on_list_graphs():
    g = TannerGraph.random_regular(120, 3, 6, seed=1)
    layer = g.layer_schedule()
    assert layer.shape == (g.m,) and layer.dtype == np.int32
    key = np.repeat(layer.astype(np.int64), 6) * g.n + g.check_lookup  # (layer, variable) of every edge
    assert np.unique(key).size == key.size
