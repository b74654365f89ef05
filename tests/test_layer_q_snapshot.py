"""The quant argument of MonteCarlo without a device: what a snapshot records and which resumes are
refused (the batches run on a stand-in executor, as tests/test_layer_snapshot.py's)."""
import pytest

from iib_project_ldpc_codes_amd import snapshot
from iib_project_ldpc_codes_amd.decoder import Quant
from iib_project_ldpc_codes_amd.graph import TannerGraph
from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo

B, ITERS = 32, 10


def _executor(first_cw, batch, stop_frame_errors, counters, stream=None):
    counters[0] += batch
    counters[1] += 1


def _mc(quant=None, schedule="layered", **kw):
    g = TannerGraph.random_regular(120, 3, 6, seed=1)
    extra = {} if quant is None else {"quant": quant}
    return MonteCarlo(g, "bsc", 0.07, ITERS, algo="minsum", alpha=0.75, seed=5, batch=B, executor=_executor,
                      schedule=schedule, **extra, **kw)


def test_only_a_quantised_run_records_the_field():
    for sched in ("flooding", "layered"):
        assert "quant" not in snapshot.config(_mc(schedule=sched))
        assert snapshot.config(_mc(schedule=sched)) == snapshot.config(_mc(schedule=sched, quant=None))
    cfg = snapshot.config(_mc(Quant(5, 7, 2.0, 8, 1)))
    assert cfg["quant"] == {"bits": 5, "post_bits": 7, "scale": 2.0, "norm8": 8, "offset": 1}
    assert {k: v for k, v in cfg.items() if k != "quant"} == snapshot.config(_mc())


def test_resume_with_the_same_quant_only(tmp_path):
    q = Quant(6, 8, 2.0)
    a = _mc(q)
    a.run(2 * B, stop_frame_errors=0)
    path = str(tmp_path / "q.json")
    snapshot.save(a.snapshot(), path)
    b = _mc(Quant(6, 8, 2.0, 6, 0))
    b.restore(snapshot.load(path))
    assert b.next_trial() == 2 * B and int(b.counters[0]) == 2 * B
    for other in (Quant(6, 8, 2.0, 6, 1), Quant(6, 8, 4.0), Quant(5, 8, 2.0), Quant(6, 7, 2.0), Quant(6, 8, 2.0, 7), None):
        with pytest.raises(ValueError):
            _mc(other).restore(snapshot.load(path))
    plain = _mc()
    plain.run(B, stop_frame_errors=0)
    with pytest.raises(ValueError):
        _mc(q).restore(plain.snapshot())
    assert snapshot.merge([a.snapshot(), a.snapshot() | {"seed": 6}])["config"]["quant"] == q.as_dict()
    with pytest.raises(ValueError):
        snapshot.merge([a.snapshot(), plain.snapshot()])


def test_what_quant_needs():
    q = Quant(6, 8, 2.0)
    with pytest.raises(ValueError):
        _mc(q, schedule="flooding")
    g = TannerGraph.random_regular(120, 3, 6, seed=1)
    with pytest.raises(ValueError):
        MonteCarlo(g, "bsc", 0.07, ITERS, algo="spa", schedule="layered", quant=q, executor=_executor)
    with pytest.raises(ValueError):
        MonteCarlo(g, "bec", 0.4, ITERS, algo="minsum", schedule="layered", quant=q, executor=_executor)
    with pytest.raises(ValueError):
        MonteCarlo.ensemble(120, 3, 6, "bsc", 0.07, ITERS, algo="minsum", schedule="layered", quant=q,
                            executor=_executor)
