"""Cases and oracle-side expectations the 64-bit trial-index tests share (tests/test_index64_ref.py on
the CPU, tests/test_gpu_index64.py on the device).

Every Monte-Carlo result is a function of the 64-bit seed, trial index and graph index; a case here
is one call whose B trials (or G graphs) straddle 2^32 under SEED, whose high word is non-zero and
whose bit 63 is set.  `expected(case, idx, seed)` is what the oracle gives for trials drawn at the
indices `idx` under `seed`: the device test compares with expected(case, true indices, SEED), and
the CPU test holds every case to telling the three bug models of `wrong_index_models` from the truth.
"""
import functools

import numpy as np

from oracle import oracle

T = 2 ** 32
M = T - 1
SEED = 0x9E3779B97F4A7C15
ALPHA, ITERS = 0.75, 5
EPS, BEC_ITERS = 0.42, 20
QUANT = (6, 8, 2.0, 6, 0)  # bits, post_bits, scale, norm8, offset
MODELS = ("index_high_dropped", "index_high_without_carry", "seed_high_dropped")


def wrong_index_models(first, B, seed):
    """{model: (indices, seed)} a kernel with the bug would draw trials first .. first + B - 1 at:
    the high word of the index dropped; the high word taken from `first` without the carry of the
    low word; the high word of the seed dropped."""
    idx = [first + b for b in range(B)]
    hi = (first >> 32) << 32
    return {"index_high_dropped": ([t & M for t in idx], seed),
            "index_high_without_carry": ([hi | (t & M) for t in idx], seed),
            "seed_high_dropped": (idx, seed & M)}


def true_indices(first, B):
    return [first + b for b in range(B)]


def _runs(idx):
    """Maximal runs (start, length) of consecutive indices."""
    out, i = [], 0
    while i < len(idx):
        j = i + 1
        while j < len(idx) and idx[j] == idx[j - 1] + 1:
            j += 1
        out.append((idx[i], j - i))
        i = j
    return out


def channel_rows(kind, p, seed, idx, n):
    """The oracle's channel words of the trials idx (any order, 64-bit)."""
    return np.concatenate([oracle.channel(kind, p, seed, s, n, c) for s, c in _runs(list(idx))])


def regular_graphs(n, dv, dc, seed, idx):
    """(check_lookup, variable_lookup, attempts) rows of the oracle's regular sampler at graphs idx."""
    parts = [oracle.sample_regular_batch(n, dv, dc, seed, s, c) for s, c in _runs(list(idx))]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def counters(curve, its, X=-1, stop=0):
    """The sequential trial loop's counters from per-trial curves [B][iters + 1] and iteration counts."""
    from tests.layered_ref import mc_counters
    return mc_counters(np.asarray(curve, np.int64), np.asarray(its, np.int64), X, stop)


# ----------------------------------------------------------------------------- graphs
@functools.lru_cache(maxsize=None)
def fixed_graph(spec):
    """(TannerGraph, csr) of new_graph(spec), kept; the device tests build their own TannerGraph (its
    device layout depends on the environment at its first use)."""
    g = new_graph(spec)
    return g, tuple(np.ascontiguousarray(a, np.int32) for a in g.to_csr())


def new_graph(spec):
    """spec: ("reg", n, seed) TannerGraph.random_regular (3,6); ("rsu", n, seed) the RSU ensemble as a
    CSR graph; ("fb", name) a tests.graph_util.FALLBACK_KERNELS graph."""
    from iib_project_ldpc_codes_amd import ensembles
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    from tests import graph_util
    kind = spec[0]
    if kind == "reg":
        return TannerGraph.random_regular(spec[1], 3, 6, seed=spec[2])
    if kind == "rsu":
        return TannerGraph.from_csr(*_rsu_csr(spec[1], spec[2]))
    assert kind == "fb"
    return TannerGraph.from_csr(*graph_util.fallback_csr(spec[1]))


@functools.lru_cache(maxsize=None)
def _rsu_csr(n, seed):
    from iib_project_ldpc_codes_amd import ensembles
    return tuple(np.asarray(a) for a in ensembles.sample_irregular(ensembles.RSU_DL4, n, seed=seed,
                                                                   deg2="zigzag").to_csr())


# ------------------------------------------------------------------------------ cases
def _case(family, name, first=T - 3, **kw):
    return dict(family=family, name=name, first=first, **kw)


CHANNEL_CASES = [_case("channel", "channel-%s" % k, kind=k, p=p, n=1003, B=8)
                 for k, p in (("bec", 0.4), ("bsc", 0.07), ("awgn", 0.8))]

# (n, B, offset of trial 2^32 in the batch, kernel): the offset lies in a workgroup after the first
# and inside a plane word (tests/test_gpu_index64.py asserts both from the plan's cw_per_wg and W)
_BITS = [(96, 40, 37, "bec_mc_bits_kernel<256,1,u32>"), (96, 65473, 101, "bec_mc_bits_kernel<256,2,u32>"),
         (96, 131072, 197, "bec_mc_bits_kernel<256,4,u32>"), (4098, 40, 37, "bec_mc_bits_kernel<512,1,u32>"),
         (26600, 10, 9, "bec_mc_bits_kernel<1024,1,u8>")]
BEC_CASES = [_case("bec", "bec-bits-%d-%d" % (n, B), first=T - off, n=n, B=B, kernel=k, X=-1, stop_after=None)
             for n, B, off, k in _BITS]
# expurgation, and a stop whose cut lies behind the crossing: the frame error that ends the run is
# the third counted one after trial 2^32 + 8 (the oracle places it)
BEC_CASES.append(_case("bec", "bec-bits-96-65473-X1-stop", first=T - 101, n=96, B=65473,
                       kernel="bec_mc_bits_kernel<256,2,u32>", X=1, stop_after=(101 + 8, 3)))
# three trials from 2^32 - 3 would end at 2^32 - 1: the batch starts at 2^32 - 1 to cross
BEC_CASES.append(_case("bec", "bec-word-107000-3", first=T - 1, n=107000, B=3, kernel="bec_kernel<1024>", X=-1,
                       stop_after=None))

BEC_ENS_CASES = [_case("bec_ens", "bec-ens-80000-2", first=T - 1, n=80000, B=2, kernel="bec_kernel<1024>"),
                 _case("bec_ens", "bec-ens-96-40", n=96, B=40, kernel="bec_peel_kernel<1024>")]

# min-sum on the BSC: (name, graph, LDPC_NO_LOC_LAYOUT, kernel, p, B); p from a scan of the oracle
# alone for 0 < frame errors < B with and without early stop (asserted in test_index64_ref.py).
# The plan (csrc/bp_plan.cpp choose_path) gives min-sum Monte-Carlo to bp_loc_kernel only on its
# one-class (3,6) shape of 512 threads (n = 10,000); (3,6) n = 1,000 decodes min-sum on
# bp_lds_kernel<3,6> with or without the local-edge layout and the RSU graph on bp_irr_kernel<lds>, so
# bp_loc_kernel's 256-thread and RSU shapes are reached by the sum-product cases below.
_SOFT = [("ms-1000", ("reg", 1000, 25), False, "bp_lds_kernel<3,6>", 0.04, 8),
         ("loc-10000", ("reg", 10000, 25), False, "bp_loc_kernel", 0.03, 8),
         ("ms-rsu-2000", ("rsu", 2000, 21), False, "bp_irr_kernel<lds>", 0.04, 8),
         ("lds-1000-noloc", ("reg", 1000, 25), True, "bp_lds_kernel<3,6>", 0.04, 8),
         ("irr-r48_256", ("fb", "r48_256"), False, "bp_irr_kernel<lds>", 0.04, 8),
         ("irr-r48_9216", ("fb", "r48_9216"), False, "bp_irr_kernel<lds+slab>", 0.04, 8),
         ("generic-r58_320", ("fb", "r58_320"), False, "bp_generic_kernel<8,lds>", 0.04, 8),
         ("generic-r58_8800", ("fb", "r58_8800"), False, "bp_generic_kernel<8,gmem>", 0.05, 4)]
SOFT_CASES = [_case("soft", "soft-" + nm, graph=g, noloc=nl, kernel=k, p=p, B=B) for nm, g, nl, k, p, B in _SOFT]

SOFT_ENS_CASES = [_case("soft_ens", "ens-200-3-6", shape=(200, 3, 6), kernel="bp_ens_kernel<8,lds>", p=0.04, B=8),
                  _case("soft_ens", "ens-90-3-9", shape=(90, 3, 9), kernel="bp_ens_kernel<16,lds>", p=0.03, B=8)]

LAYER_CASES = [_case("layer", "layer-r36_600", graph="r36_600", lds=True, kernel="bp_layer_kernel<8,lds>", p=0.06, B=8),
               _case("layer", "layer-r58_8800", graph="r58_8800", lds=False, kernel="bp_layer_kernel<8,gmem>", p=0.074,
                     B=8)]
LAYER_Q_CASES = [_case("layer_q", "layerq-r36_602", graph="r36_602", kernel="bp_layer_q_kernel<8>", p=0.06, B=8),
                 _case("layer_q", "layerq-r324_1024", graph="r324_1024", kernel="bp_layer_q_kernel<32>", p=0.008, B=8)]

# sum-product on the BSC: (name, graph, LDPC_NO_LOC_LAYOUT, kernel, threads of the plan)
_SPA = [("loc-1000", ("reg", 1000, 25), False, "bp_loc_kernel", 256),
        ("loc-10000", ("reg", 10000, 25), False, "bp_loc_kernel", 512),
        ("loc-rsu-2000", ("rsu", 2000, 21), False, "bp_loc_kernel", 256),
        ("lds-1000-noloc", ("reg", 1000, 25), True, "bp_lds_kernel<3,6>", 256)]
SPA_CASES = [_case("spa", "spa-" + nm, graph=g, noloc=nl, kernel=k, threads=t, p=0.07, B=8) for nm, g, nl, k, t in _SPA]

ML_CASES = [_case("ml", "ml-fixed-200", n=200, ens=False, B=16), _case("ml", "ml-ens-100", n=100, ens=True, B=16)]
ML_EPS, ML_ITERS = 0.42, 20

SEQ_E = 8192  # the sequential-draw sampler's smallest edge count (csrc/sampler.hip kSeqMinE)
SAMPLER_CASES = [_case("sampler", "sample-reg-1000-3-6", kind="regular", n=1000, dv=3, dc=6, B=6),
                 _case("sampler", "sample-reg-96-4-8", kind="regular", n=96, dv=4, dc=8, B=6),
                 _case("sampler", "sample-seq-2732", kind="regular", n=2732, dv=3, dc=6, B=6),
                 _case("sampler", "sample-seq-10000", kind="regular", n=10000, dv=3, dc=6, B=6),
                 _case("sampler", "sample-seq-2732-G300", first=T - 150, kind="regular", n=2732, dv=3, dc=6, B=300),
                 _case("sampler", "sample-csr-2000", kind="csr", n=2000, B=6),
                 _case("sampler", "sample-csr-20000", kind="csr", n=20000, B=6),
                 _case("sampler", "sample-csr-30000", kind="csr", n=30000, B=6)]

DRIVER_CASE = _case("layer_q", "driver-layerq-r36_600", first=T - 96, graph="r36_600", p=0.06, B=192)

ALL_CASES = (CHANNEL_CASES + BEC_CASES + BEC_ENS_CASES + SOFT_CASES + SOFT_ENS_CASES + LAYER_CASES + LAYER_Q_CASES
             + SPA_CASES + ML_CASES + SAMPLER_CASES + [DRIVER_CASE])
BY_NAME = {c["name"]: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)
# the modes a soft Monte-Carlo case runs in: early stop off / on
MODES = (False, True)


# ------------------------------------------------------------------------ expectations
CH_KIND = {"bec": oracle.CH_BEC, "bsc": oracle.CH_BSC, "awgn": oracle.CH_AWGN}


def _bec_curves(words, iters, g):
    _, err, its = oracle.bec_decode_batch(words, iters, g.variable_lookup, g.check_lookup, g.n, g.k, g.dv, g.dc)
    return np.concatenate([np.count_nonzero(words == 2, axis=1)[:, None], err], axis=1), its


def bec_stop(c, curve):
    """The stop_frame_errors of a case with stop_after = (trial offset, extra): the counted frame errors
    of the trials up to that offset, plus extra."""
    if c["stop_after"] is None:
        return 0
    off, extra = c["stop_after"]
    f = curve[:off + 1, -1]
    return int(((f > c["X"]) & (f != 0)).sum()) + extra


def _minsum_curves(csr, llr, early_stop):
    """Per-trial error curves [B][ITERS + 1] and iteration counts of the oracle's flooding min-sum, one
    decode per iteration count (tests/test_gpu_parity.py::test_mc_minsum_bsc_exact)."""
    B = llr.shape[0]
    curve = np.zeros((B, ITERS + 1), np.int64)
    curve[:, 0] = (llr < 0).sum(axis=1)
    for t in range(1, ITERS + 1):
        _, h, its = oracle.bp_decode_batch(csr, llr, t, 1, alpha=ALPHA, early_stop=early_stop)
        curve[:, t] = h.sum(axis=1)
    return curve, its.astype(np.int64)


def _expected(c, idx, seed):
    fam = c["family"]
    if fam == "channel":
        return (channel_rows(CH_KIND[c["kind"]], c["p"], seed, idx, c["n"]),)
    if fam == "bec":
        g = fixed_graph(("reg", c["n"], 11))[0]
        curve, its = _bec_curves(channel_rows(oracle.CH_BEC, EPS, seed, idx, c["n"]), BEC_ITERS, g)
        stop = bec_stop(c, curve)
        return counters(curve, its, c["X"], stop), np.array([stop], np.int64)
    if fam == "bec_ens":
        n = c["n"]
        words = channel_rows(oracle.CH_BEC, EPS, seed, idx, n)
        chk, var, _ = regular_graphs(n, 3, 6, seed, idx)
        curve = np.zeros((len(idx), BEC_ITERS + 1), np.int64)
        its = np.zeros(len(idx), np.int64)
        for t in range(len(idx)):
            _, err, its[t] = oracle.message_passing(words[t], BEC_ITERS, var[t], chk[t], n, n // 2, 3, 6)
            curve[t] = np.insert(err, 0, int(np.count_nonzero(words[t] == 2)))
        return curve, its
    if fam == "soft":
        csr = fixed_graph(c["graph"])[1]
        llr = channel_rows(oracle.CH_BSC, c["p"], seed, idx, csr[2].size - 1)
        return tuple(counters(*_minsum_curves(csr, llr, es)) for es in MODES)
    if fam == "soft_ens":
        n, dv, dc = c["shape"]
        llr = channel_rows(oracle.CH_BSC, c["p"], seed, idx, n)
        chk, var, _ = regular_graphs(n, dv, dc, seed, idx)
        out = []
        for es in MODES:
            rows = [_minsum_curves(oracle.csr_from_lists(var[b], chk[b], n, n * dv // dc, dv, dc), llr[b:b + 1], es)
                    for b in range(len(idx))]
            out.append(counters(np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])))
        return tuple(out)
    if fam in ("layer", "layer_q"):
        from tests import layered_q_ref, layered_ref, layered_util
        csr = layered_util.graph_csr(c["graph"])
        layer = layered_util.layers(c["graph"])[1]
        llr = channel_rows(oracle.CH_BSC, c["p"], seed, idx, csr[2].size - 1)
        out = []
        for es in MODES:
            if fam == "layer":
                r = layered_ref.decode(csr, layer, llr, ITERS, 1, ALPHA, es)
            else:
                r = layered_q_ref.decode(csr, layer, llr, ITERS, *QUANT, early_stop=es)
            out.append(counters(r[3], r[2]))
        return tuple(out)
    if fam == "spa":
        csr = fixed_graph(c["graph"])[1]
        llr = channel_rows(oracle.CH_BSC, c["p"], seed, idx, csr[2].size - 1)
        return (np.array([len(idx), int((llr < 0).sum())], np.int64),)
    if fam == "ml":
        return (_ml_counters(c, idx, seed),)
    if fam == "sampler":
        if c["kind"] == "regular":
            return regular_graphs(c["n"], c["dv"], c["dc"], seed, idx)
        vptr, cptr = csr_ptrs(c["n"])
        rows = [oracle.sample_csr(vptr, cptr, seed, g) for g in idx]
        return tuple(np.array([r[k] for r in rows]) for k in range(3))
    raise KeyError(fam)


def csr_ptrs(n):
    from iib_project_ldpc_codes_amd import ensembles
    return ensembles.degree_ptrs(ensembles.RSU_DL4, n)


def _ml_counters(c, idx, seed):
    """[trials, MP frame errors, MP bit errors, ML frame errors, ML bit errors | MP curve], the
    sequential loop of tests/test_gpu_ml.py::_oracle_mc without a stop."""
    n, m = c["n"], c["n"] // 2
    words = channel_rows(oracle.CH_BEC, ML_EPS, seed, idx, n).astype(np.uint8)
    if c["ens"]:
        chk, var, _ = regular_graphs(n, 3, 6, seed, idx)
        cptr = np.arange(m + 1, dtype=np.int32) * 6
    else:
        g = fixed_graph(("reg", n, 9))[0]
        cptr, cvar = g.to_csr()[:2]
    out = np.zeros(5 + ML_ITERS + 1, np.int64)
    for t in range(len(idx)):
        cv, v2c = (chk[t], var[t]) if c["ens"] else (cvar, g.variable_lookup)
        _, err, _ = oracle.bec_decode_batch(words[t][None], ML_ITERS, v2c, cv, n, n - m, 3, 6)
        e = np.concatenate([[int((words[t] == 2).sum())], err[0]])
        _, uns = oracle.ml_decode_batch(cptr, cv, words[t], n, m)
        out[0] += 1
        out[1] += e[-1] != 0
        out[2] += e[-1]
        out[3] += uns[0] > 0
        out[4] += uns[0]
        out[5:] += e
    return out


_cache = {}


def expected(c, idx, seed):
    """Tuple of arrays: what the oracle gives case c for trials (graphs) at indices idx under seed;
    kept per (case, indices, seed), read-only."""
    key = (c["name"], hash(tuple(idx)), len(idx), idx[0], idx[-1], seed)
    if key not in _cache:
        out = _expected(c, idx, seed)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def want(c):
    return expected(c, true_indices(c["first"], c["B"]), SEED)
