"""The reference side of tests/test_gpu_sampler_shapes.py (CPU only): the cases of
tests/sampler_shapes_util.py reach every kernel the samplers' launch plan can name, stay within
the attempt cap on the oracle alone, yield simple graphs whose two lists name the same edges, and
would each see the bug they are there for -- small numpy restatements of the bug applied to the
oracle's output change it.
"""
import numpy as np
import pytest

from tests import sampler_shapes_util as u


def _names(p):
    return {p["draw"], p["var_side"], p["search"]} - {"none"}


def test_cases_reach_every_kernel_the_plan_names():
    """The union of the cases' plan names equals what the plan emits over the sweep of
    tests/test_sample_plan.py: a kernel that drops out of the cases turns this red."""
    got = set()
    for c in u.CASES:
        got |= _names(u.case_plan(c))
    assert got == u.sweep_names() and len(got) == 13


def test_cases_hold_every_mode():
    """Each mode of the launch at least once: counter widths 2 / 4 / 8 / none, both ring and row
    widths, mdv as a reciprocal and as 0, one chunk and several, odd E on the sequential sampler,
    the three one-level kernels, and a search pass with fewer workgroups than graphs."""
    plans = {c["name"]: u.case_plan(c) for c in u.CASES}
    seq = [p for p in plans.values() if p["seq"]]
    assert {p["fb"] for p in seq} == {0, 2, 4, 8}
    assert {p["ring"] for p in seq} == {2, 4} and {p["row"] for p in seq} == {2, 4}
    assert {p["mdv"] == 0 for p in seq if "regular" in p["draw"]} == {True, False}
    assert {p["nch"] == 1 for p in seq if p["V"]} == {True, False}
    assert any(p["V"] == 0 and p["emit_fb"] == 0 for p in seq)
    assert any(p["seq"] and u.case_E(c) % 2 for c, p in ((c, plans[c["name"]]) for c in u.CASES))
    assert {p["K"] for p in plans.values() if not p["seq"]} == {256, 512, 1024}
    assert {u.case_E(c) for c in u.CASES} >= {8190, 8192, 8193, 393216, 393220}
    b = u.BIG
    p = u.regular_plan(b["n"], b["dv"], b["dc"], b["G"])
    assert (p["draw"], p["row"], p["lds"], p["per_cu"], p["W"]) == (u.SEQ_RI, 4, 52576, 3, 768) and p["W"] < b["G"]


@pytest.mark.parametrize("c", u.CASES, ids=[c["name"] for c in u.CASES])
def test_case_plan_cap_and_graphs(c):
    p = u.case_plan(c)
    for k, v in c["plan"].items():
        assert p[k] == v, (c["name"], k, p)
    chk, var, att = u.want(c)
    assert np.all(att > 0) and np.all(att <= u.ATTEMPT_CAP), att
    E = u.case_E(c)
    if c["kind"] == "regular":
        n, dv, dc = c["n"], c["dv"], c["dc"]
        vptr, cptr = np.arange(n + 1) * dv, np.arange(E // dc + 1) * dc
    else:
        vptr, cptr = u.case_ptrs(c)
        n = len(vptr) - 1
    check_of_slot = np.repeat(np.arange(len(cptr) - 1), np.diff(cptr))
    var_of_row = np.repeat(np.arange(n), np.diff(vptr))
    for g in range(c["G"]):
        assert chk[g].min() >= 0 and chk[g].max() < n
        np.testing.assert_array_equal(np.bincount(chk[g], minlength=n), np.diff(vptr))  # the degree structure
        edges = np.unique(check_of_slot.astype(np.int64) * n + chk[g])
        assert edges.size == E  # simple: no check holds a variable twice
        # the variable side names the same edges, each row ascending
        if c["kind"] == "regular":
            back = var[g].astype(np.int64) * n + var_of_row  # entries are check ids
            assert np.all(np.diff(var[g].reshape(n, dv), axis=1) > 0) or dv == 1
        else:
            np.testing.assert_array_equal(chk[g][var[g]], var_of_row)  # entries are slot ids
            back = check_of_slot[var[g]].astype(np.int64) * n + var_of_row
            inner = np.ones(E, bool)
            inner[vptr[:-1][np.diff(vptr) > 0]] = False  # a row's first entry has no predecessor in it
            assert np.all(np.diff(var[g])[inner[1:]] > 0)
        np.testing.assert_array_equal(np.sort(back), edges)


def test_big_case_stays_within_the_cap():
    chk, var, att = u.big_want()
    assert chk.shape == (32, 393216) and np.all(att > 0) and np.all(att <= u.ATTEMPT_CAP)
    assert len({a.tobytes() for a in chk}) == 32  # 32 different graphs


def _csr_form(c, g, last_check_tested):
    """Graph g of a regular case drawn through the oracle's CSR form with the same degree
    structure -- the same stream -- and, on demand, the last check split into dc checks of
    degree 1, which no test can reject: the sampler whose division by dc is one check short."""
    from oracle import oracle
    n, dv, dc = c["n"], c["dv"], c["dc"]
    E = n * dv
    cptr = np.arange(E // dc + 1) * dc
    if not last_check_tested:
        cptr = np.concatenate((cptr[:-1], np.arange(E - dc + 1, E + 1)))
    return oracle.sample_csr(np.arange(n + 1) * dv, cptr, u.REG_SEED, g)


@pytest.mark.parametrize("c", u.DIVISION, ids=[c["name"] for c in u.DIVISION])
def test_division_windows_hold_graphs_that_need_the_last_check(c):
    """Each window stays within the cap and holds what it is there for: drawn without a test of
    the graph's last check, the named graphs (and only they) take an earlier attempt and come out
    different, so a device whose slot / dc is one check short at E misses the oracle there.  A
    change of the stream, the seed or the window that loses this turns the test red."""
    chk, var, att = u.division_want(c["name"])
    dc = c["dc"]
    assert chk.shape == (c["G"], c["n"] * c["dv"]) and np.all(att > 0) and np.all(att <= u.ATTEMPT_CAP)
    assert u.regular_plan(c["n"], c["dv"], dc, c["G"])["seq"] and dc & (dc - 1)
    seen = []
    for k in range(c["G"]):
        g = c["first"] + k
        cv, vs, a = _csr_form(c, g, True)  # the CSR form is the same draw
        np.testing.assert_array_equal(cv, chk[k])
        np.testing.assert_array_equal(vs // dc, var[k])
        assert a == att[k]
        wcv, _, wa = _csr_form(c, g, False)
        assert 0 < wa <= a
        if wa < a:
            assert not np.array_equal(wcv, cv)
            pair = wcv[-dc:]
            assert len(set(pair.tolist())) < dc  # the accepted attempt's last check holds a variable twice
            assert all(len(set(row.tolist())) == dc for row in wcv[:-dc].reshape(-1, dc))  # and no other does
            seen.append(g)
        else:
            np.testing.assert_array_equal(wcv, cv)
    assert seen == c["needs_last_check"]


def test_table_cases_do_not_see_a_short_division():
    """The six graphs of the table's dc = 3 and dc = 7 cases have no attempt that only the last
    check rejects: they hold `mdc` to nothing more than the plan; the DIVISION windows do."""
    for name in ("reg-2731-3-3", "reg-9555-3-7"):
        c = u.BY_NAME[name]
        att = u.want(c)[2]
        for k in range(c["G"]):
            assert _csr_form(c, u.REG_FIRST + k, False)[2] == att[k]


# ------------------------------------------------------------------------- bug models
def _var_side_with_wrapping_counters(c, chk, bits):
    """The variable side as the device's counters build it (sample_var_side_kernel, slots taken
    in order): counters of `bits` bits packed into 32-bit words, each slot adds one to its
    variable's counter and lands at the rank the counter held, then every row is sorted.  A
    counter that receives 2^bits adds carries into its neighbour's (the next variable's, within a
    word), whose ranks then run past its row; an entry never written stays -1."""
    if c["kind"] == "regular":
        vptr, dc = np.arange(c["n"] + 1) * c["dv"], c["dc"]  # rows of check ids
    else:
        vptr, dc = u.case_ptrs(c)[0], 1  # rows of slot ids
    out = np.full(chk.size + 512, -1, np.int64)  # (room for ranks past the last row)
    words = [0] * ((len(vptr) * bits + 31) // 32 + 1)
    for x, v in enumerate(chk.tolist()):
        pos = v * bits
        old = words[pos >> 5]
        words[pos >> 5] = (old + (1 << (pos & 31))) & 0xFFFFFFFF
        out[vptr[v] + ((old >> (pos & 31)) & ((1 << bits) - 1))] = x // dc
    out = out[:chk.size]
    for v in range(len(vptr) - 1):
        out[vptr[v]:vptr[v + 1]].sort()
    return out


@pytest.mark.parametrize("name,narrower", [("csr-vhub15", 2), ("reg-600-16-2", 4), ("csr-vhub255", 4), ("reg-2048-4-4", 2)])
def test_hub_cases_see_a_wrapping_counter(name, narrower):
    """A counter one step narrower than the plan's overflows on the hub variable and changes the
    variable side; at the plan's width the restatement is the oracle's list.  (Degree 16 on 4 bits
    still ranks 0..15 rightly and only carries into the next variable's counter, which shows when
    that variable has occurrences left: certain at (600, 16, 2), where every variable is a hub,
    but a matter of slot order for the single hub of csr-vhub16.)"""
    c = u.BY_NAME[name]
    fb = u.case_plan(c)["fb"]
    chk, var, _ = u.want(c)
    for g in range(c["G"]):
        np.testing.assert_array_equal(_var_side_with_wrapping_counters(c, chk[g], fb), var[g])
        assert not np.array_equal(_var_side_with_wrapping_counters(c, chk[g], narrower), var[g])


def test_regular_counter_cases_see_a_wrapping_counter():
    """(640, 15, 2) and (600, 16, 2): every variable is a hub.  15 occurrences fit 4 bits, 16 do
    not (and 4 do not fit 2 bits at (2048, 4, 4))."""
    for name, fb, narrower in (("reg-2048-4-4", 4, 2), ("reg-640-15-2", 4, 2), ("reg-600-16-2", 8, 4)):
        c = u.BY_NAME[name]
        assert u.case_plan(c)["fb"] == fb and c["dv"] < 1 << fb and c["dv"] >= 1 << narrower


@pytest.mark.parametrize("name", [c["name"] for c in u.CASES])
def test_16_bit_ids_change_exactly_the_wide_cases(name):
    """Variable ids taken mod 2^16 change the check side exactly where the plan has the int ring
    or the int32 permutation; check ids (regular) or slot ids (CSR) mod 2^16 change the variable
    side exactly where the plan stages int32 rows."""
    c = u.BY_NAME[name]
    p = u.case_plan(c)
    chk, var, _ = u.want(c)
    wide_ids = p["ring"] == 4 if p["seq"] else p["draw"] == u.ONE1024 and int(chk.max()) >= 65536
    assert all(np.any(chk[g] != chk[g] % 65536) for g in range(c["G"])) == bool(wide_ids), (name, int(chk.max()))
    if p["seq"] and p["V"]:
        assert all(np.any(var[g] != var[g] % 65536) for g in range(c["G"])) == (p["row"] == 4), (name, int(var.max()))
    if name == "reg-65536-3-6":
        assert int(chk.max()) == 65535  # the largest id a u16 ring holds
    if name == "reg-98304-2-3":
        assert int(var.max()) == 65535  # the largest check id a u16 row holds


@pytest.mark.parametrize("name", ["reg-2731-3-3", "reg-9555-3-7", "reg-2048-4-4", "reg-640-15-2", "reg-8192-1-2"])
def test_reciprocal_of_dc_arithmetic(name):
    """The arithmetic behind the DIVISION windows only (what a case sees of it is held by
    test_division_windows_hold_graphs_that_need_the_last_check): slot / dc by multiply-high needs
    ceil(2^32 / dc), exact over the whole range of the sampler; with the floor, a dc that is no
    power of two gives one check too few at every multiple of dc, E among them -- the graph's
    last check would go untested."""
    c = u.BY_NAME[name]
    dc, E = c["dc"], u.case_E(c)
    x = np.arange(0, 393216 + 1, dtype=np.uint64)
    ceil_r, floor_r = -(-(1 << 32) // dc), (1 << 32) // dc
    np.testing.assert_array_equal((x * np.uint64(ceil_r)) >> np.uint64(32), x // np.uint64(dc))
    wrong = int((np.uint64(E) * np.uint64(floor_r)) >> np.uint64(32))
    if dc & (dc - 1):
        assert wrong == E // dc - 1
    else:
        assert wrong == E // dc  # a power of two: both reciprocals are 2^32 / dc
