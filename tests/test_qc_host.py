"""Quasi-cyclic codes without a device: the description (iib_project_ldpc_codes_amd/qc.py), the
library's expansion and block-row schedule (ldpc_debug_qc_expand) against an independent numpy
expansion (tests/qc_ref.py), and what a snapshot records."""
import numpy as np
import pytest

from iib_project_ldpc_codes_amd import _native, decoder, qc, snapshot
from iib_project_ldpc_codes_amd.graph import TannerGraph
from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
from tests import qc_ref
from tests.layered_util import schedule
from tests.qc_util import HAND_Z31, code
from tests.test_layer_snapshot import _executor

MASK_4x12 = np.asarray(HAND_Z31) < 0
NAMES = ["arr36_z7", "arr36_z67", "rnd36_z64", "rnd36_z65", "hand_z31", "dense2x12_z37", "dense2x20_z23", "z1"]


@pytest.mark.parametrize("name", NAMES)
def test_expansion_equals_the_numpy_expansion(name):
    c = code(name)
    cptr, cvar, vptr, vslot, layer = c.expand()
    want = qc_ref.csr(c.base, c.Z)
    for got, w in zip((cptr, cvar, vptr, vslot), want):
        np.testing.assert_array_equal(got, w)
    # the slot order is the ascending block-column order, a variable's slots ascend with the check
    for chk in range(c.m):
        assert np.all(np.diff(cvar[cptr[chk]:cptr[chk + 1]] // c.Z) > 0)
    assert all(np.all(np.diff(vslot[vptr[v]:vptr[v + 1]]) > 0) for v in range(c.n))
    # check r Z + i holds c Z + (i + s) mod Z
    for r in range(c.mb):
        cols = np.nonzero(c.base[r] >= 0)[0]
        for i in (0, c.Z // 2, c.Z - 1):
            np.testing.assert_array_equal(cvar[cptr[r * c.Z + i]:cptr[r * c.Z + i + 1]],
                                          cols * c.Z + (i + c.base[r, cols]) % c.Z)
    # the block rows are the layers, and no two checks of a layer share a variable
    np.testing.assert_array_equal(layer, np.arange(c.m) // c.Z)
    H = qc_ref.dense(c.base, c.Z).astype(np.int64)
    for r in range(c.mb):
        assert H[r * c.Z:(r + 1) * c.Z].sum(axis=0).max() <= 1
    g = c.graph()
    np.testing.assert_array_equal(g.layer_schedule(), layer)
    np.testing.assert_array_equal(g.parity_check(), H)
    assert g.layer_rule == "qc/block-row/v1" == decoder.layer_rule(g)
    assert snapshot.graph_fingerprint(g) == snapshot.graph_fingerprint(TannerGraph.from_csr(*want))


def _four_cycle_free(c):
    H = qc_ref.dense(c.base, c.Z).astype(np.int64)
    G = H @ H.T
    np.fill_diagonal(G, 0)
    return G.max() <= 1


def test_constructors_have_no_four_cycle():
    assert _four_cycle_free(qc.array_code(3, 6, 7)) and _four_cycle_free(qc.array_code(3, 6, 67))
    # Z = 7 is the smallest (3,6) size there is: the cell-by-cell draw gets through at seed 2 and is stuck at seed 1
    assert _four_cycle_free(qc.random_base(3, 6, 7, seed=2)) and _four_cycle_free(qc.random_base(3, 6, 67, seed=1))
    with pytest.raises(RuntimeError):
        qc.random_base(3, 6, 7, seed=1)
    masked = qc.random_base(4, 12, 31, seed=3, mask=MASK_4x12)
    np.testing.assert_array_equal(masked.base < 0, MASK_4x12)
    assert _four_cycle_free(masked) and _four_cycle_free(code("hand_z31"))
    np.testing.assert_array_equal(qc.random_base(3, 6, 67, seed=1).base, qc.random_base(3, 6, 67, seed=1).base)
    assert np.any(qc.random_base(3, 6, 67, seed=1).base != qc.random_base(3, 6, 67, seed=2).base)
    a = qc.array_code(3, 6, 1667)
    assert (a.n, a.m) == (10002, 5001) and a.base[2, 5] == 10
    with pytest.raises(RuntimeError):
        qc.random_base(3, 6, 2, seed=1)  # two shifts cannot keep six columns apart


def test_refusals():
    L = _native.lib()

    def create(base, Z):
        b = np.ascontiguousarray(base, np.int32)
        return L.ldpc_debug_qc_expand(b.shape[0], b.shape[1], Z, b.ctypes.data, None, None, None, None, None)

    ok = [[0, 1, -1], [2, -1, 0]]
    assert create(ok, 3) == 0
    qc.QCCode(ok, 3)
    bad = [(ok, 0), (ok, -4), ([[0, 3, -1], [2, -1, 0]], 3), ([[0, -2, -1], [2, 1, 0]], 3),
           ([[0, 1, 2], [-1, -1, -1]], 3), ([[0, -1, 1], [2, -1, 0]], 3), ([[0] * 33, [1] * 33], 2)]
    for base, Z in bad:
        assert create(base, Z) == _native.LDPC_EINVAL, (base, Z)
        with pytest.raises(ValueError):
            qc.QCCode(base, Z)
    assert create([[0] * 32], 1) == 0
    for dv, dc, Z in ((3, 6, 9), (3, 6, 5), (3, 6, 1)):  # not prime; below dc
        with pytest.raises(ValueError):
            qc.array_code(dv, dc, Z)


def test_text_round_trip(tmp_path):
    c = code("hand_z31")
    path = str(tmp_path / "base.txt")
    c.to_text(path)
    back = qc.QCCode.from_text(path, 31)
    np.testing.assert_array_equal(back.base, c.base)
    assert back.Z == 31 and open(path).read().split() == [str(x) for x in c.base.ravel()]
    with open(path, "a") as f:
        f.write("1 2\n")
    with pytest.raises(ValueError):
        qc.QCCode.from_text(path, 31)
    c.to_text(path)
    with pytest.raises(ValueError):
        qc.QCCode.from_text(path, 30)  # a shift of 30 needs Z > 30


def test_other_graphs_keep_their_colouring():
    """The expansion taken as a plain CSR graph is coloured as before; the rule's name stands."""
    c = code("hand_z31")  # block rows 0 and 1 share no block column: first fit puts them into one layer
    rc, L, layer = schedule(c.expand()[:4])
    assert rc == 0 and L < c.mb and np.any(layer != np.arange(c.m) // c.Z)
    assert _native.lib().ldpc_layer_rule().decode() == snapshot.LAYER_RULE == decoder.layer_rule()
    plain = TannerGraph.from_csr(*c.expand()[:4])
    assert decoder.layer_rule(plain) == snapshot.LAYER_RULE
    assert _native.lib().ldpc_graph_layer_rule(None).decode() == snapshot.LAYER_RULE


def _mc(graph, schedule="layered"):
    return MonteCarlo(graph, "bsc", 0.05, 10, algo="minsum", alpha=0.75, seed=5, batch=32, executor=_executor,
                      schedule=schedule)


def test_snapshot_records_the_block_row_rule(tmp_path):
    g = code("arr36_z67").graph()
    plain = TannerGraph.from_csr(*g.csr)
    assert snapshot.config(_mc(plain))["layer_rule"] == snapshot.LAYER_RULE
    assert "layer_rule" not in snapshot.config(_mc(g, "flooding"))
    assert snapshot.config(_mc(g, "flooding")) == snapshot.config(_mc(plain, "flooding"))
    a = _mc(g)
    a.run(64, stop_frame_errors=0)
    path = str(tmp_path / "qc.json")
    snapshot.save(a.snapshot(), path)
    snap = snapshot.load(path)
    assert snap["config"]["layer_rule"] == "qc/block-row/v1" and snap["config"]["schedule"] == "layered"
    b = _mc(code("arr36_z67").graph())
    b.restore(snap)
    assert b.next_trial() == 64
    with pytest.raises(ValueError):  # the same edges under the colouring decode differently
        _mc(plain).restore(snap)
    with pytest.raises(ValueError):
        _mc(g).restore(_mc(plain).snapshot())
