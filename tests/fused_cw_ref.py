"""Numpy reference of the fused codeword Monte-Carlo of the fixed-point decoders
(include/ldpc_mi355x.h, ldpc_mc_layered_q_cw_batch_dev), and the cases of tests/test_gpu_mc_fused_cw.py.
Nothing here touches the device.

The chain per trial: information bits (codeword_util.info_bits) -> tests/encode_ref.py -> the oracle's
BSC stream, reflected where the codeword bit is 1 -> rate_match_ref.apply_rules -> layered_q_ref.decode
with the posteriors of every iteration -> per-iteration counts against the codeword under the count
mask: row[0] over the transmitted, counted positions on the sign of the float, row[t] over the counted
ones on the sign of the posterior after iteration t (a stopped frame keeps its posteriors).

Cases (seed 7, trials 0 .. B - 1, 20 iterations; B = 64):
  A  r36_96 with rate_match_ref.classes (6 known, 8 punctured), QUANT: the table kernel <8>
  B  qc.random_base(3, 6, 17, 5), n = 102 (no multiple of 4), block column 0 punctured, QUANT:
     bp_qc_q_kernel<64,8>, and the table kernel under qc_util.table_kernels()
  C  qc.random_base(3, 6, 307, 5), n = 1,842 (Z > 256: two checks per thread), block column 0
     punctured, QUANT: bp_qc_q_kernel<256,8>
  D  the code of C, every position transmitted (no description), quantiser (6, 8, 2.0, 6, 0)

E-H hold the codeword mode at the other widths (tests/qc_util.py has the codes; QUANT, block column 0
punctured, the words built as case B's with the information bits at shortened positions zeroed first):
  E  rnd3x12_z37, n = 444: bp_qc_q_kernel<64,16>.  n is a multiple of 4 (the one-dword codeword load)
     and not of 32 (a partial plane word)
  F  rnd3x20_z61, n = 1,220: bp_qc_q_kernel<64,32>, two-word records (the plane at rec + 2 m).  305
     words of P > 4 * 64: the masked count's second round, with a ragged tail
  G  mix3x12_z67, n = 804, block column 9 shortened: bp_qc_q_kernel<256,16> with block rows of degree
     12, 9 and 5 (absent edges while the plane is live), a KNOWN class on a quasi-cyclic kernel
  H  rnd3x20_z257, n = 5,140, block column 16 shortened: bp_qc_q_kernel<256,32>.  1,285 words of P >
     4 * 256; Z = 257 is two checks per thread with a tail of one
Under qc_util.table_kernels() the same cases run bp_layer_q_kernel<16> (E, G) and <32> (F, H).
(E, F and H have rank m - 2, as regular circulant bases do; G is full rank.  The shortened block
columns lie wholly in the encoder's information positions: case() asserts it.)

Count masks of case G (MASKS; rows(count=)): None is the description's default ("codeword": what is
not known, 737 positions);
  "mod3"  count[v] = (v % 3 != 0): 536 positions, known and punctured ones among them, transmitted
          ones left out
  "info"  RateMatch(count="info"): the encoder's information positions that are not known, 536
"""
import functools

import numpy as np

from oracle import oracle
from tests import codeword_util as cu, encode_ref, layered_q_ref, qc_util, rate_match_ref as rr

B = 64
QUANT_D = (6, 8, 2.0, 6, 0)
QC_NAME = {"B": "rnd36_z17", "C": "rnd36_z307", "D": "rnd36_z307", "E": "rnd3x12_z37", "F": "rnd3x20_z61",
           "G": "mix3x12_z67", "H": "rnd3x20_z257"}
SHORT_COLS = {"G": [9], "H": [16]}  # shortened block columns; block column 0 is punctured in every case but D
MASKS = (None, "mod3", "info")
# [trials, frame errors, bit errors, iterations, curve[0]] of (case, p, early stop, count mask), worked
# out on the CPU before the assertions were written; tests/test_fused_cw_host.py re-derives them
FIGURES = {("E", 0.02, True, None): [64, 32, 531, 835, 495], ("F", 0.01, True, None): [64, 41, 962, 981, 750],
           ("G", 0.015, True, None): [64, 32, 286, 791, 618], ("G", 0.015, False, None): [64, 32, 286, 1280, 618],
           ("H", 0.008, True, None): [64, 15, 786, 763, 2379], ("H", 0.008, False, None): [64, 15, 786, 1280, 2379],
           ("G", 0.015, True, "mod3"): [64, 31, 194, 791, 416], ("G", 0.015, True, "info"): [64, 32, 215, 791, 419]}
CURVE_1_4 = {("G", None): [725, 641, 433, 378], ("G", "mod3"): [488, 448, 299, 264]}
P_OF = {"E": 0.02, "F": 0.01, "G": 0.015, "H": 0.008}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(csr, layer, n, cls (None: no description), x uint8 [B, n] read-only, quant) of a case."""
    if name == "A":
        return dict(csr=cu.csr("r36_96"), layer=cu.layers("r36_96"), n=96, cls=rr.classes("r36_96"),
                    x=rr.codewords("r36_96", B), quant=cu.QUANT)
    from iib_project_ldpc_codes_amd import encoder
    g = qc_util.graph(QC_NAME[name])
    Z = g.code.Z
    cptr, cvar = g.csr[0], g.csr[1]
    _, info, par, _ = encoder.host_description(cptr, cvar, g.n)
    cls = None
    if name != "D":
        cls = np.zeros(g.n, np.uint8)
        cls[:Z] = rr.PUNCT  # block column 0
        for c in SHORT_COLS.get(name, ()):
            cls[c * Z:(c + 1) * Z] = rr.KNOWN
    u = cu.info_bits(cu.SEED, 0, B, info.size)
    if name in SHORT_COLS:  # a shortened bit is an information bit, fixed to 0 before encoding
        short = np.flatnonzero(cls == rr.KNOWN)
        assert np.isin(short, info).all(), "a shortened position is a parity position of the encoder"
        u[:, np.isin(info, short)] = 0
    x = encode_ref.solve(encode_ref.parity_matrix(cptr, cvar, g.n), info, par, u)
    if name in SHORT_COLS:
        assert not x[:, short].any() and x.any()
    x.setflags(write=False)
    return dict(csr=tuple(np.ascontiguousarray(a, np.int32) for a in g.csr), layer=g.layer_schedule(), n=g.n, cls=cls,
                x=x, quant=cu.QUANT if name != "D" else QUANT_D)


def rows_of(csr, layer, cls, x, llr0, quant, iters, early_stop, known_llr=rr.KNOWN_LLR, count=None):
    """(rows int64 [B][iters + 1], its [B], ties) of the words x on the all-zero stream llr0 float32
    [B, n]; ties: how often a counted posterior is 0 where the codeword bit is 1, over iterations
    1 .. iters (the positions the all-zero shortcut would count as correct).  count: a 0/1 mask [n],
    None the description's default (rate_match_ref.default_count)."""
    x = np.asarray(x, np.uint8)
    cls = np.zeros(x.shape[1], np.uint8) if cls is None else np.asarray(cls)
    cnt = (rr.default_count(cls) if count is None else np.asarray(count)).astype(bool)
    assert cnt.shape == cls.shape
    llr = rr.apply_rules(np.where(x == 1, -llr0, llr0).astype(np.float32), cls, x, False, known_llr)
    res = layered_q_ref.decode(csr, layer, llr, iters, *quant, early_stop=early_stop, at=range(iters + 1))
    rows = np.zeros((x.shape[0], iters + 1), np.int64)
    ties = 0
    for t in range(1, iters + 1):
        post = res[t][0].astype(np.int32)
        rows[:, t] = (((post < 0) != (x == 1)) & cnt[None, :]).sum(axis=1)
        ties += int(((post == 0) & (x == 1) & cnt[None, :]).sum())
    if iters == 0:  # the one entry: the final count, of the quantised channel values
        rows[:, 0] = (((res[0][0].astype(np.int32) < 0) != (x == 1)) & cnt[None, :]).sum(axis=1)
    else:
        rows[:, 0] = (((llr < 0) != (x == 1)) & (cnt & (cls == rr.TX))[None, :]).sum(axis=1)
    return rows, np.asarray(res[iters][2], np.int64), ties


@functools.lru_cache(maxsize=None)
def mask(name, count):
    """The count mask uint8 [n] of a case, read-only: None (the default), "mod3" or "info" (MASKS)."""
    c = case(name)
    cls = np.zeros(c["n"], np.uint8) if c["cls"] is None else c["cls"]
    if count is None:
        out = rr.default_count(cls)
    elif count == "mod3":
        out = (np.arange(c["n"]) % 3 != 0).astype(np.uint8)
    else:
        assert count == "info"
        from iib_project_ldpc_codes_amd import encoder
        info = encoder.host_description(c["csr"][0], c["csr"][1], c["n"])[1]
        out = np.zeros(c["n"], np.uint8)
        out[info] = 1
        out &= cls != rr.KNOWN
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rows(name, p, early_stop, iters=cu.ITERS, count=None, zero=False):
    """rows_of a case on the oracle's BSC stream of crossover probability p (exact against the device);
    count: a mask of MASKS; zero: the all-zero word in place of the case's words."""
    c = case(name)
    llr0 = oracle.channel(oracle.CH_BSC, p, cu.SEED, 0, c["n"], B)
    x = np.zeros((B, c["n"]), np.uint8) if zero else c["x"]
    out = rows_of(c["csr"], c["layer"], c["cls"], x, llr0, c["quant"], iters, early_stop,
                  count=None if count is None else mask(name, count))
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


def counters(name, p, early_stop, X=-1, stop=0, iters=cu.ITERS, count=None, zero=False):
    """The counter vector [trials, frame errors, bit errors, iterations | curve] of one batch."""
    r, its, _ = rows(name, p, early_stop, iters, count, zero)
    return layered_q_ref.mc_counters(np.asarray(r), np.asarray(its), X, stop)


@functools.lru_cache(maxsize=None)
def plain_counters(name, p, early_stop):
    """The counter vector of a case's code with no description and no codeword (every position
    transmitted and counted, the all-zero word) under cu.QUANT: what the codeword mode and the all-zero
    entry ldpc_mc_layered_q_batch_dev must both give."""
    c = case(name)
    llr0 = oracle.channel(oracle.CH_BSC, p, cu.SEED, 0, c["n"], B)
    zero = np.zeros((B, c["n"]), np.uint8)
    r, its, _ = rows_of(c["csr"], c["layer"], None, zero, llr0, cu.QUANT, cu.ITERS, early_stop)
    return layered_q_ref.mc_counters(r, its, -1, 0)


# ------------------------------------------------------------------ the plans of the codeword mode
def _plans(entry, head, calls, cus, has_desc, rc_only):
    from iib_project_ldpc_codes_amd import _native
    from tests.layered_q_util import Q_KEYS
    args = np.ascontiguousarray([[B_, iters, algo, es, mc, post] for algo, es, mc, post, iters, B_ in calls],
                                np.int32).reshape(len(calls), 6)
    out = np.zeros((len(calls), 9), np.int64)
    names = np.zeros((len(calls), 64), np.uint8)
    rc = getattr(_native.lib(), entry)(*head, len(calls), args.ctypes.data, cus, int(has_desc), out.ctypes.data,
                                       names.ctypes.data)
    if rc_only:
        return rc
    assert rc == 0, _native.last_error()
    plans = [dict(zip(Q_KEYS, (int(v) for v in row))) for row in out]
    for p, nm in zip(plans, names):
        p["name"] = nm.tobytes().split(b"\0")[0].decode()
    return plans


def layer_q_cw_plans(csr, calls, has_desc, cus=256, rc_only=False):
    """ldpc_debug_layer_q_cw_plan (host only) of `calls` = (algo, early_stop, mc, want_post, iters, B)
    tuples on one CSR graph, as layered_q_util.layer_q_plans."""
    cptr, cvar, vptr, vslot = [np.ascontiguousarray(a, np.int32) for a in csr]
    head = (cptr.ctypes.data, cvar.ctypes.data, vptr.ctypes.data, vslot.ctypes.data, vptr.size - 1, cptr.size - 1)
    return _plans("ldpc_debug_layer_q_cw_plan", head, calls, cus, has_desc, rc_only)


def qc_cw_plans(c, calls, has_desc, cus=256, rc_only=False):
    """ldpc_debug_qc_cw_plan (host only) of a QCCode, as qc_util.qc_plans."""
    return _plans("ldpc_debug_qc_cw_plan", (c.mb, c.nb, c.Z, c.base.ctypes.data), calls, cus, has_desc, rc_only)


def curve_bytes(iters):
    """The Monte-Carlo curve of iters + 1 ints, padded to 16 bytes."""
    return 16 * ((4 * (iters + 1) + 15) // 16)


def plane_bytes(n):
    """One bit per variable, in whole words."""
    return 4 * ((n + 31) // 32)
