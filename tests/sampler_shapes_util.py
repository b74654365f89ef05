"""The sampler shapes of tests/test_sampler_shapes_ref.py (CPU) and tests/test_gpu_sampler_shapes.py
(GPU): one list of cases, each with the launch-plan fields (csrc/sample_plan.cpp, read through
ldpc_debug_sample_plan) it is there for, and the oracle's graphs for it, computed once.

Regular cases draw graphs 1000.. at seed 31, CSR cases graphs 50.. at seed 8.  Every case stays
within ATTEMPT_CAP attempts per graph on the oracle alone (the library retries up to 2^20 times:
a shape that practically never yields a simple graph would hold a device for its whole time limit).
"""
import functools

import numpy as np

from oracle import oracle

ATTEMPT_CAP = 20000
REG_SEED, REG_FIRST = 31, 1000
CSR_SEED, CSR_FIRST = 8, 50
CUS = 256  # the CU count the literal plan rows are written for (an MI355X)

PLAN_KEYS = ("seq", "threads", "K", "lds", "bw", "ring", "fb", "fbu", "emit_fb", "mdv", "V", "nch", "row", "vs_lds",
             "per_cu", "W")


def sample_plan(n, m, E, max_cdeg, max_vdeg, regular, dv, G, cus=CUS):
    """The sampler's launch plan (ldpc_debug_sample_plan, host only) as a dict: PLAN_KEYS and the
    three kernel names draw / var_side / search."""
    from iib_project_ldpc_codes_amd import _native
    out = np.zeros(16, np.int64)
    names = np.zeros((3, 64), np.uint8)
    rc = _native.lib().ldpc_debug_sample_plan(n, m, E, max_cdeg, max_vdeg, int(regular), dv, G, cus, out.ctypes.data,
                                              names.ctypes.data)
    assert rc == 0, _native.last_error()
    p = dict(zip(PLAN_KEYS, (int(x) for x in out)))
    for key, nm in zip(("draw", "var_side", "search"), names):
        p[key] = nm.tobytes().split(b"\0")[0].decode()
    return p


def regular_plan(n, dv, dc, G, cus=CUS):
    return sample_plan(n, n * dv // dc, n * dv, dc, dv, True, dv, G, cus)


def csr_plan(vptr, cptr, G, cus=CUS):
    return sample_plan(len(vptr) - 1, len(cptr) - 1, int(vptr[-1]), int(np.diff(cptr).max()), int(np.diff(vptr).max()),
                       False, 0, G, cus)


def sweep_shapes():
    """A few thousand argument tuples of sample_plan across every threshold: regular (dv, dc)
    shapes the public entry admits, and CSR shapes as (n, m, E, max_cdeg, max_vdeg)."""
    out = []
    ns = (60, 64, 600, 2730, 2731, 4096, 5462, 8192, 16384, 21846, 24576, 24640, 32768, 65536, 65537, 65538, 98304,
          98307, 131072, 131074, 196608, 196610, 300000)
    for n in ns:
        for dv, dc in ((1, 2), (2, 2), (2, 3), (2, 4), (3, 3), (3, 6), (3, 7), (4, 4), (4, 8), (15, 2), (16, 2), (3, 192),
                       (3, 193), (255, 3), (256, 3)):
            if n * dv % dc == 0 and n * dv < 1 << 30:
                out += [(n, n * dv // dc, n * dv, dc, dv, True, dv, G, cus) for G in (1, 6, 800, 10000)
                        for cus in (0, 256, 304)]
    for E in (6000, 8191, 8192, 12000, 16384, 16385, 30000, 65535, 65536, 65537, 90000, 393216, 393217, 500000):
        for n in (63, 6000, 45000, 65536, 65537, 200000):
            for cdeg in (3, 192, 193):
                for vdeg in (2, 3, 4, 15, 16, 255, 256, 1000):
                    out += [(n, max(1, E // 3), E, cdeg, vdeg, False, 0, G, cus) for G, cus in ((3, 256), (800, 304), (5, 0))]
    return out


@functools.lru_cache(maxsize=None)
def sweep_plans():
    """((arguments, plan), ...) over sweep_shapes()."""
    return tuple((s, sample_plan(*s)) for s in sweep_shapes())


def sweep_names():
    """Every kernel name the plan emits over the sweep (draw, variable-side and search kernels)."""
    return {p[k] for _, p in sweep_plans() for k in ("draw", "var_side", "search")} - {"none"}


# ------------------------------------------------------------------- CSR degree structures
def _ptr(deg):
    return np.concatenate(([0], np.cumsum(deg))).astype(np.int32)


def hub_checks(E, d):
    """Variables of degree 2; checks of degree 3 plus four of degree d at the start, 1/3, 2/3 and
    the end (E - 4 d a multiple of 3, E even)."""
    k = E - 4 * d
    assert k % 3 == 0 and E % 2 == 0
    cdeg = np.full(k // 3 + 4, 3, np.int64)
    cdeg[[0, len(cdeg) // 3, 2 * len(cdeg) // 3, len(cdeg) - 1]] = d
    return _ptr(np.full(E // 2, 2)), _ptr(cdeg)


def hub_variable(n, d, at=1000):
    """Variable `at` of degree d, the other n - 1 of degree 2; checks of degree 3."""
    vdeg = np.full(n, 2, np.int64)
    vdeg[at] = d
    E = int(vdeg.sum())
    assert E % 3 == 0
    return _ptr(vdeg), _ptr(np.full(E // 3, 3))


def empty_rows():
    """Degree-0 variables (the first, two in the middle, the last) and a check of degree 1 and
    one of degree 0 among variables of degree 2 and checks of degree 3: E = 12,001."""
    vdeg = np.full(6004, 2, np.int64)
    vdeg[[0, 2000, 2001, 6003]] = 0
    vdeg[3000] = 3
    cdeg = np.full(4001, 3, np.int64)
    cdeg[1500], cdeg[2500], cdeg[4000] = 1, 0, 6
    assert vdeg.sum() == cdeg.sum() == 12001
    return _ptr(vdeg), _ptr(cdeg)


def wide_ids(n, E, k):
    """n variables of which only every k-th has sockets (degree 2, the rest degree 0); checks of
    degree 3: variable ids past 2^16 with few sockets."""
    vdeg = np.zeros(n, np.int64)
    vdeg[::k][:E // 2] = 2
    assert vdeg.sum() == E and E % 3 == 0
    return _ptr(vdeg), _ptr(np.full(E // 3, 3))


# ---------------------------------------------------------------------------- the cases
SEQ_RU, SEQ_RI = "sample_seq_kernel<regular,u16>", "sample_seq_kernel<regular,int>"
SEQ_CU, SEQ_CI = "sample_seq_kernel<csr,u16>", "sample_seq_kernel<csr,int>"
ONE256, ONE512, ONE1024 = ("sample_regular_kernel<256,u16,lds>", "sample_regular_kernel<512,u16,lds>",
                           "sample_regular_kernel<1024,int32,gmem>")
VS16, VS32 = "sample_var_side_kernel<1024,u16>", "sample_var_side_kernel<1024,int32>"


def _reg(n, dv, dc, why, G=6, **plan):
    return dict(name=f"reg-{n}-{dv}-{dc}", kind="regular", n=n, dv=dv, dc=dc, G=G, why=why, plan=plan)


def _csr(name, make, why, G=3, host=True, **plan):
    return dict(name=name, kind="csr", make=make, G=G, why=why, host=host, plan=plan)


# plan: the fields the case is there for (asserted from ldpc_debug_sample_plan before any device work)
CASES = [
    _reg(4095, 2, 3, "below 8,192: one level, K = 256", draw=ONE256, K=256, seq=0),
    _reg(2730, 3, 6, "the same side at (3,6)", draw=ONE256, K=256, seq=0),
    _reg(4096, 2, 4, "E = 8,192 exactly: sequential; n a multiple of 64, one chunk", draw=SEQ_RU, bw=256, fb=2,
         nch=1, var_side=VS16),
    _reg(2731, 3, 3, "smallest sequential shape with odd E, dc = 3", draw=SEQ_RU, fb=2),
    _reg(9555, 3, 7, "odd E, dc = 7: the multiply-high division by dc", draw=SEQ_RU, fb=2),
    _reg(8192, 1, 2, "dv = 1: mdv = 0, the true divide", draw=SEQ_RU, mdv=0, fb=2),
    _reg(2048, 4, 4, "4-bit occurrence counters", draw=SEQ_RU, fb=4),
    _reg(640, 15, 2, "the widest 4-bit counter, dc = 2", draw=SEQ_RU, fb=4),
    _reg(600, 16, 2, "the narrowest 8-bit counter, dc = 2", draw=SEQ_RU, fb=8),
    _reg(5462, 3, 6, "E just past 16,384: still sequential", draw=SEQ_RU, nch=2),
    _reg(21846, 3, 6, "E just past 65,536: still sequential, two chunks", draw=SEQ_RU, nch=2, row=2),
    _reg(65536, 3, 6, "u16 ring holding id 65,535", G=2, draw=SEQ_RU, ring=2, search="sample_search_kernel<regular,u16>"),
    _reg(65538, 3, 6, "int ring", G=2, draw=SEQ_RI, ring=4, row=2, search="sample_search_kernel<regular,int>"),
    _reg(65537, 2, 2, "the smallest n past the u16 ring (and m past the u16 rows)", G=2, draw=SEQ_RI, ring=4, row=4),
    _reg(131074, 1, 2, "m = 65,537: the smallest m past the u16 rows; dv = 1 under an int ring", G=2, draw=SEQ_RI,
         mdv=0, row=4, var_side=VS32),
    _reg(98304, 2, 3, "m = 65,536: 16-bit rows under an int ring", draw=SEQ_RI, ring=4, row=2, var_side=VS16),
    _reg(98307, 2, 3, "m = 65,538: 32-bit rows", draw=SEQ_RI, ring=4, row=4, var_side=VS32),
    _reg(131072, 3, 6, "E = 393,216 exactly: the largest bitmap", G=2, draw=SEQ_RI, bw=12288, lds=52576),
    _reg(196610, 2, 4, "E = 393,220: one level in global memory", draw=ONE1024, K=1024, seq=0),
    _reg(131074, 3, 6, "the same kernel at (3,6)'s rejection rate", G=2, draw=ONE1024, K=1024, seq=0),
    _csr("csr-hub192-12000", lambda: hub_checks(12000, 192), "degree-192 checks across round boundaries",
         draw=SEQ_CU, row=2, search="sample_search_kernel<csr,u16>"),
    _csr("csr-hub192-30000", lambda: hub_checks(30000, 192), "the same, E = 30,000", draw=SEQ_CU, row=2),
    _csr("csr-hub192-90000", lambda: hub_checks(90000, 192), "the same, 32-bit CSR rows", draw=SEQ_CU, row=4,
         var_side=VS32),
    # (up to 5,486 attempts of a 256-thread workgroup, seconds per call: the device entry alone)
    _csr("csr-hub193-11998", lambda: hub_checks(11998, 193), "check degree 193: one level, K = 256", host=False,
         draw=ONE256, K=256),
    _csr("csr-hub193-29998", lambda: hub_checks(29998, 193), "check degree 193: one level, K = 512", draw=ONE512, K=512),
    _csr("csr-hub193-89998", lambda: hub_checks(89998, 193), "check degree 193: one level, K = 1024", draw=ONE1024,
         K=1024),
    _csr("csr-vhub15", lambda: hub_variable(5995, 15), "a variable of degree 15: 4-bit counters", draw=SEQ_CU, fb=4),
    _csr("csr-vhub16", lambda: hub_variable(5993, 16), "a variable of degree 16: 8-bit counters", draw=SEQ_CU, fb=8),
    _csr("csr-vhub255", lambda: hub_variable(5875, 255), "a variable of degree 255: 8-bit counters, 256-variable chunks",
         draw=SEQ_CU, fb=8, V=256, nch=23),
    _csr("csr-vhub256", lambda: hub_variable(5873, 256), "a variable of degree 256: global CAS after the sequential draw",
         draw=SEQ_CU, fb=0, V=0, emit_fb=0, var_side="none"),
    _csr("csr-empty-rows", empty_rows, "degree-0 variables, checks of degree 0 and 1, odd E", draw=SEQ_CU),
    _csr("csr-int-ring", lambda: hub_variable(66000, 2), "66,000 variables: the CSR form's int ring", draw=SEQ_CI,
         ring=4, row=4, search="sample_search_kernel<csr,int>"),
    _csr("csr-wide-ids-6000", lambda: wide_ids(66000, 6000, 22), "ids past 2^16 below 8,192 sockets: 1024 buckets",
         draw=ONE1024, K=1024, lds=65600),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# G > W: one _dev call of 800 graphs on (196608, 2, 4) -- E = 393,216, int ring, 32-bit rows,
# 52,576 bytes of LDS, so three search workgroups per CU: W = 768 on 256 CUs
BIG = dict(n=196608, dv=2, dc=4, G=800, part=100,
           compared=sorted(set(range(8)) | set(range(792, 800)) | set(range(29, 800, 49))))
assert len(BIG["compared"]) == 32


# slot / dc by multiply-high (the number of checks whose slots are all drawn): a reciprocal that
# is one too small -- floor instead of ceil(2^32 / dc) -- loses the last check at every multiple
# of dc, so the graph's last check is never tested.  That shows only in a graph with an attempt
# whose last check alone holds a variable twice, ahead of its first simple attempt: about one
# graph in a thousand at these shapes.  These windows hold such graphs (needs_last_check;
# tests/test_sampler_shapes_ref.py asserts it by drawing each graph through the oracle's CSR form
# with the last check split into checks of degree 1, which nothing can reject).
DIVISION = [dict(name="div-2731-3-3", kind="regular", n=2731, dv=3, dc=3, first=REG_FIRST + 368, G=32,
                 needs_last_check=[1371, 1396]),
            dict(name="div-9555-3-7", kind="regular", n=9555, dv=3, dc=7, first=REG_FIRST + 95, G=1,
                 needs_last_check=[1095])]


@functools.lru_cache(maxsize=None)
def division_want(name):
    c = next(c for c in DIVISION if c["name"] == name)
    out = oracle.sample_regular_batch(c["n"], c["dv"], c["dc"], REG_SEED, c["first"], c["G"])
    for a in out:
        a.setflags(write=False)
    return out


def case_ptrs(c):
    """(var_ptr, check_ptr) of a CSR case."""
    return _case_ptrs(c["name"])


@functools.lru_cache(maxsize=None)
def _case_ptrs(name):
    vptr, cptr = BY_NAME[name]["make"]()
    vptr.setflags(write=False)
    cptr.setflags(write=False)
    return vptr, cptr


def case_plan(c, cus=CUS):
    if c["kind"] == "regular":
        return regular_plan(c["n"], c["dv"], c["dc"], c["G"], cus)
    return csr_plan(*case_ptrs(c), c["G"], cus)


def case_E(c):
    return c["n"] * c["dv"] if c["kind"] == "regular" else int(case_ptrs(c)[0][-1])


@functools.lru_cache(maxsize=None)
def _want(name):
    c = BY_NAME[name]
    if c["kind"] == "regular":
        out = oracle.sample_regular_batch(c["n"], c["dv"], c["dc"], REG_SEED, REG_FIRST, c["G"])
    else:
        vptr, cptr = case_ptrs(c)
        rows = [oracle.sample_csr(vptr, cptr, CSR_SEED, CSR_FIRST + g) for g in range(c["G"])]
        out = tuple(np.stack([np.asarray(r[k]) for r in rows]) for k in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def want(c):
    """The oracle's (check side [G][E], variable side [G][E], attempts [G]) of a case, computed
    once and read-only."""
    return _want(c["name"])


@functools.lru_cache(maxsize=None)
def big_want():
    """The oracle's graphs BIG['compared'] of the G > W case, in that order."""
    rows = [oracle.sample_regular(BIG["n"], BIG["dv"], BIG["dc"], REG_SEED, REG_FIRST + g) for g in BIG["compared"]]
    out = tuple(np.stack([np.asarray(r[k]) for r in rows]) for k in range(3))
    for a in out:
        a.setflags(write=False)
    return out
