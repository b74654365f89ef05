"""Host-only checks of the layered decoder's schedule (csrc/graph_host.cpp build_layer_schedule)
through ldpc_debug_layer_schedule, and of the reference the GPU tests hold the kernel to
(tests/layered_ref.py): no device needed.

* The schedule is a proper colouring of the check-conflict graph on the (3,6) n = 600 and
  n = 10,000 graphs and every graph of graph_util.FALLBACK_KERNELS: every check in exactly one of
  the layers 0..L-1, none empty, no two checks of a layer sharing a variable, L within the
  first-fit bound max_cdeg (max_vdeg - 1) + 1, the same schedule from two calls.
* The balancing step keeps first fit's number of layers and evens them out (the largest layer of
  the headline graph within 10 % of the mean; plain first fit leaves 883 .. 5 checks there).
* A check that holds a variable twice, an empty check and check degree 33 have no schedule
  (LDPC_EUNSUP).
* The reference's check rules against oracle.check_update at degrees 2-32, with +-0 and values
  beyond the 23 ln 2 clamp among the inputs: min-sum bit for bit, sum-product within one fp32 ulp.
"""
import numpy as np
import pytest

from oracle import oracle
from tests import layered_ref
from tests.graph_util import FALLBACK_KERNELS, csr_from_checks
from tests.layered_util import graph, graph_csr, layers, schedule

GRAPHS = ["r36_600", "r36_10000"] + list(FALLBACK_KERNELS)
LDPC_EUNSUP = -5


def _first_fit(csr):
    """Plain first fit in check order: the sizes of its layers."""
    cptr, cvar = csr[0], csr[1]
    n = csr[2].size - 1
    used = [set() for _ in range(n)]  # layers already holding a check of the variable
    sizes = []
    for c in range(cptr.size - 1):
        vs = cvar[cptr[c]:cptr[c + 1]]
        taken = set().union(*(used[v] for v in vs))
        l = next(i for i in range(len(sizes) + 1) if i not in taken)
        if l == len(sizes):
            sizes.append(0)
        sizes[l] += 1
        for v in vs:
            used[v].add(l)
    return sizes


@pytest.mark.parametrize("name", GRAPHS)
def test_schedule_is_a_proper_colouring(name):
    csr = graph_csr(name)
    cptr, cvar, vptr = csr[0], csr[1], csr[2]
    m, n = cptr.size - 1, vptr.size - 1
    L, layer = layers(name)
    assert layer.shape == (m,)  # every check has its one layer ...
    assert layer.min() == 0 and layer.max() == L - 1
    assert np.all(np.bincount(layer, minlength=L) > 0)  # ... none of 0..L-1 is empty
    # no two checks of a layer share a variable: (layer, variable) pairs of all edges are distinct
    key = np.repeat(layer.astype(np.int64), np.diff(cptr)) * n + cvar
    assert np.unique(key).size == key.size
    assert L <= int(np.diff(cptr).max()) * (int(np.diff(vptr).max()) - 1) + 1
    rc, L2, layer2 = schedule(csr)
    assert rc == 0 and L2 == L
    np.testing.assert_array_equal(layer2, layer)
    np.testing.assert_array_equal(graph(name).layer_schedule(), layer)  # the public method


@pytest.mark.parametrize("name", ["r36_600", "r36_10000", "r58_8800", "mixA"])
def test_balancing_keeps_the_layer_count_and_evens_the_layers(name):
    csr = graph_csr(name)
    ff = _first_fit(csr)
    L, layer = layers(name)
    sizes = np.bincount(layer, minlength=L)
    assert L == len(ff)
    assert sizes.max() <= max(ff)
    print(name, "first fit", ff, "balanced", sizes.tolist())
    if name == "r36_10000":
        assert max(ff) > 2 * min(ff)  # what the step is for
        assert sizes.max() <= 1.10 * (csr[0].size - 1) / L


def test_rule_name_is_the_one_snapshots_record():
    from iib_project_ldpc_codes_amd import decoder, snapshot
    assert decoder.layer_rule() == snapshot.LAYER_RULE


def _rows_csr(rows, n):
    cptr = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
    return csr_from_checks(cptr, np.concatenate([np.asarray(r, np.int32) for r in rows]), n)


def test_graphs_without_a_schedule():
    from iib_project_ldpc_codes_amd import _native
    # a check that holds variable 0 twice
    rc, _, _ = schedule(_rows_csr([[0, 0, 1], [1, 2, 3], [2, 3, 0]], 4))
    assert rc == LDPC_EUNSUP and "layer schedule" in _native.last_error()
    # check 0 of degree 33 (tests/test_bp_plan.py's deg33)
    rows = [np.arange(33)] + [np.array([i, 33 + 3 * i, 34 + 3 * i, 35 + 3 * i]) for i in range(33)]
    rc, _, _ = schedule(_rows_csr(rows, 33 + 99))
    assert rc == LDPC_EUNSUP
    # the same graph with check 0 cut to 32 variables has one (variable 32 then hangs on check 33 alone)
    rc, L, layer = schedule(_rows_csr([np.arange(32)] + rows[1:], 33 + 99))
    assert rc == 0 and L >= 2 and layer[0] != layer[1]
    # an empty check
    csr = _rows_csr([[0, 1], [1, 2], [2, 0]], 3)
    cptr = np.concatenate((csr[0], csr[0][-1:])).astype(np.int32)
    rc, _, _ = schedule((cptr,) + tuple(csr[1:]))
    assert rc == LDPC_EUNSUP


def _rule_inputs(d, rs):
    x = (rs.randn(64, d) * rs.choice([0.5, 3.0, 12.0], size=(64, 1))).astype(np.float32)
    u = rs.rand(64, d)
    x = np.where(u < 0.06, 0.0, x)
    x = np.where((u >= 0.06) & (u < 0.12), -0.0, x)
    x = np.where((u >= 0.12) & (u < 0.18), np.sign(x) * 40.0, x)    # beyond the clamp
    x = np.where((u >= 0.18) & (u < 0.21), np.sign(x) * 1e30, x)
    x[0] = x[0, 0]        # every magnitude tied
    x[1] = np.abs(x[1])
    return np.ascontiguousarray(x, np.float32)


@pytest.mark.parametrize("d", list(range(2, 33)))
def test_reference_rules_against_the_oracle(d):
    rs = np.random.RandomState(100 + d)
    x = _rule_inputs(d, rs)
    ms = layered_ref.check_update_ms(x, 0.75)
    spa = layered_ref.check_update_spa(x)
    for b in range(x.shape[0]):
        want = oracle.check_update(x[b], 1, 0.75)
        np.testing.assert_array_equal(ms[b].view(np.uint32), want.view(np.uint32), err_msg=str(x[b]))
        want = oracle.check_update(x[b], 0)
        assert np.all(np.abs(spa[b].astype(np.float64) - want) <= np.spacing(np.abs(want))), (x[b], spa[b], want)
