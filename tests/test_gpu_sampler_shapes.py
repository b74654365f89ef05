"""The device samplers against the oracle at the shapes that select each kernel and mode of their
launch (csrc/sampler.hip launch_sample, planned by csrc/sample_plan.cpp): the cases of
tests/sampler_shapes_util.py.  Each case first holds the call to the kernels its plan names
(ldpc_debug_sample_plan with this device's CU count; tests/test_sample_plan.py holds the plan
itself) and to the attempt cap on the oracle alone (tests/test_sampler_shapes_ref.py), then
compares both lists and the attempt counts of the host entry and of the device entry with the
oracle's, bit for bit: everything here is an integer, there is no tolerance anywhere.
"""
import numpy as np
import pytest

from oracle import oracle
from tests import sampler_shapes_util as u

pytestmark = pytest.mark.gpu

SENTINEL = -7


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lib():
    from iib_project_ldpc_codes_amd import _native
    return _native, _native.lib()


def _held(c, cus):
    """The case's plan fields on this device, and the oracle's graphs within the attempt cap."""
    p = u.case_plan(c, cus)
    for k, v in c["plan"].items():
        assert p[k] == v, (c["name"], k, p)
    if p["seq"]:
        assert p["W"] == min(c["G"], cus * p["per_cu"]) > 0 and p["search"] != "none", p
    want = u.want(c)
    assert np.all(want[2] > 0) and np.all(want[2] <= u.ATTEMPT_CAP)
    return want


def _host(c, G):
    """The host entry on sentinel-filled arrays: (check side, variable side, attempts)."""
    _native, L = _lib()
    E = u.case_E(c)
    a, b, att = (np.full(s, SENTINEL, np.int32) for s in ((G, E), (G, E), G))
    if c["kind"] == "regular":
        rc = L.ldpc_sample_regular(c["n"], c["dv"], c["dc"], u.REG_SEED, u.REG_FIRST, G, a.ctypes.data, b.ctypes.data,
                                   att.ctypes.data)
    else:
        vptr, cptr = u.case_ptrs(c)
        rc = L.ldpc_sample_csr(len(vptr) - 1, len(cptr) - 1, vptr.ctypes.data, cptr.ctypes.data, u.CSR_SEED, u.CSR_FIRST, G,
                               a.ctypes.data, b.ctypes.data, att.ctypes.data)
    _native.check(rc, "ldpc_sample_" + c["kind"])
    return a, b, att


def _dev(torch, c, G, first=None, offset=0):
    """The device entry on sentinel-filled tensors whose lists start `offset` int32 into their
    allocations (one guard word behind each): (check side, variable side, attempts) and the two
    whole allocations."""
    _native, L = _lib()
    E = u.case_E(c)
    raw = [torch.full((G * E + offset + 1,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2)]
    a, b = (r[offset:offset + G * E].view(G, E) for r in raw)
    att = torch.full((G,), SENTINEL, dtype=torch.int32, device="cuda")
    assert a.data_ptr() == raw[0].data_ptr() + 4 * offset
    s = torch.cuda.current_stream().cuda_stream
    if c["kind"] == "regular":
        rc = L.ldpc_sample_regular_dev(c["n"], c["dv"], c["dc"], u.REG_SEED, u.REG_FIRST if first is None else first, G,
                                       a.data_ptr(), b.data_ptr(), att.data_ptr(), s)
    else:
        vptr, cptr = u.case_ptrs(c)
        rc = L.ldpc_sample_csr_dev(len(vptr) - 1, len(cptr) - 1, vptr.ctypes.data, cptr.ctypes.data, u.CSR_SEED,
                                   u.CSR_FIRST if first is None else first, G, a.data_ptr(), b.data_ptr(), att.data_ptr(), s)
    _native.check(rc, f"ldpc_sample_{c['kind']}_dev")
    torch.cuda.synchronize()
    return (a, b, att), raw


def _equal(got, want, what):
    for g, w, side in zip(got, want, ("check side", "variable side", "attempts")):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {side}")


@pytest.mark.parametrize("c", u.CASES, ids=[c["name"] for c in u.CASES])
def test_case_matches_oracle(torch, cus, c):
    want = _held(c, cus)
    if c.get("host", True):
        _equal(_host(c, c["G"]), want, "host entry")
    got, raw = _dev(torch, c, c["G"])
    _equal([t.cpu().numpy() for t in got], want, "device entry")
    assert all(int(r[-1]) == SENTINEL for r in raw)  # nothing written behind the lists


@pytest.mark.parametrize("name", ["reg-2731-3-3", "csr-empty-rows"])
def test_odd_rows_from_a_4_byte_aligned_base(torch, cus, name):
    """Odd E: every other row of the lists starts on a 4-byte boundary, where the paired stores of
    the sequential draw are no longer 8-byte aligned.  With the lists one int32 into their
    allocations row 0 is such a row as well; the word in front and the word behind stay."""
    c = u.BY_NAME[name]
    want = _held(c, cus)
    assert u.case_E(c) % 2 == 1 and u.case_plan(c, cus)["seq"]
    got, raw = _dev(torch, c, c["G"], offset=1)
    assert got[0].data_ptr() % 8 == 4 and got[1].data_ptr() % 8 == 4
    _equal([t.cpu().numpy() for t in got], want, "offset lists")
    assert all(int(r[0]) == SENTINEL and int(r[-1]) == SENTINEL for r in raw)


@pytest.mark.parametrize("c", u.DIVISION, ids=[c["name"] for c in u.DIVISION])
def test_windows_that_need_the_last_check_tested(torch, cus, c):
    """dc = 3 and 7: graphs with an attempt that only the graph's last check rejects, ahead of their
    first simple one (sampler_shapes_util.DIVISION) -- a division by dc that is one check short at
    the multiples of dc accepts that attempt."""
    p = u.regular_plan(c["n"], c["dv"], c["dc"], c["G"], cus)
    assert p["draw"] == u.SEQ_RU and c["dc"] & (c["dc"] - 1)
    want = u.division_want(c["name"])
    assert np.all(want[2] > 0) and np.all(want[2] <= u.ATTEMPT_CAP)
    got, _ = _dev(torch, c, c["G"], first=c["first"])
    _equal([t.cpu().numpy() for t in got], want, c["name"])


def test_more_graphs_than_search_workgroups(torch, cus):
    """(196608, 2, 4), G = 800 in one call: the search pass has fewer persistent workgroups than
    graphs, so a workgroup is home to several graphs and its pool row (a variable_lookup row) is
    rebuilt behind it.  The same graphs drawn 100 per call are identical on the device, and 32 of
    them -- the first and last eight and 16 in between -- equal the oracle's."""
    b = u.BIG
    c = dict(kind="regular", n=b["n"], dv=b["dv"], dc=b["dc"])
    p = u.regular_plan(b["n"], b["dv"], b["dc"], b["G"], cus)
    assert p["draw"] == u.SEQ_RI and p["row"] == 4 and p["per_cu"] == 3
    assert 0 < p["W"] == 3 * cus < b["G"], p  # a device of 267 CUs or more would need a larger G here
    want = u.big_want()
    assert np.all(want[2] > 0) and np.all(want[2] <= u.ATTEMPT_CAP)
    whole, raw = _dev(torch, c, b["G"])
    assert all(int(r[-1]) == SENTINEL for r in raw)
    for k in range(0, b["G"], b["part"]):
        part, _ = _dev(torch, c, b["part"], first=u.REG_FIRST + k)
        for w, q in zip(whole, part):
            assert torch.equal(w[k:k + b["part"]], q), k
        del part
    idx = torch.tensor(b["compared"], device="cuda")
    _equal([t[idx].cpu().numpy() for t in whole], want, "G = 800")


# ------------------------------------------------------------------------ downstream
def test_bec_ensemble_on_a_2_4_sequential_shape(torch, cus):
    """ldpc_mc_ensemble_batch_dev at (4096, 2, 4), B = 96: the sampler draws into the workspace's
    own lists (E = 8,192: the sequential sampler, not the (3,6) checks' packed validation) and the
    erasure decoder reads them; counters equal the oracle's sampler plus message_passing."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    n, dv, dc, B, iters, eps, seed = 4096, 2, 4, 96, 20, 0.3, 17
    assert u.regular_plan(n, dv, dc, B, cus)["draw"] == u.SEQ_RU
    chk, var, att = oracle.sample_regular_batch(n, dv, dc, seed, 0, B)
    assert np.all(att > 0) and np.all(att <= u.ATTEMPT_CAP)
    words = oracle.channel(oracle.CH_BEC, eps, seed, 0, n, B)
    want = np.zeros(4 + iters + 1, np.int64)
    for b in range(B):
        _, err, it = oracle.message_passing(words[b], iters, var[b], chk[b], n, n - n * dv // dc, dv, dc)
        curve = np.insert(err, 0, int(np.count_nonzero(words[b] == 2)))
        want += np.concatenate(([1, curve[-1] != 0, curve[-1], it], curve))
    assert 10 < want[1] < B - 10  # decoded and failed frames, from the oracle alone
    mc = MonteCarlo.ensemble(n, dv, dc, "bec", eps, iters, seed=seed, batch=B)
    mc.run_batch(0, B)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mc.counters.cpu().numpy(), want)


@pytest.mark.parametrize("early_stop", [True, False])
def test_soft_ensemble_on_a_4_4_sequential_shape(torch, cus, early_stop):
    """ldpc_mc_ensemble_soft_batch_dev, min-sum on the BSC, at (2048, 4, 4), B = 64: graphs from
    the sequential sampler with 4-bit occurrence counters; every counter and curve entry exact."""
    from tests import test_gpu_ens_soft as s
    from tests.test_ens_plan import ens_plans
    shape, B, p, seed, iters = (2048, 4, 4), 64, 0.2, 17, 20
    plan = u.regular_plan(*shape, B, cus)
    assert plan["draw"] == u.SEQ_RU and plan["fb"] == 4
    rc, plans = ens_plans(*shape, [(1, int(early_stop), 1, 0, iters, B)])
    assert rc == 0 and plans[0]["name"] == "bp_ens_kernel<8,lds>"
    curve, its = s._oracle_trials(shape, p, seed, B, iters, early_stop)
    want = s._counters(curve, its)
    assert want[0] == B and 5 <= want[1] <= B - 5  # decoded and failed frames, from the oracle alone
    np.testing.assert_array_equal(s._mc(shape, "bsc", p, seed, B, iters, "minsum", early_stop), want)
