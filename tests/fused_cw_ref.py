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
"""
import functools

import numpy as np

from oracle import oracle
from tests import codeword_util as cu, encode_ref, layered_q_ref, qc_util, rate_match_ref as rr

B = 64
QUANT_D = (6, 8, 2.0, 6, 0)
QC_NAME = {"B": "rnd36_z17", "C": "rnd36_z307", "D": "rnd36_z307"}


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
    x = encode_ref.solve(encode_ref.parity_matrix(cptr, cvar, g.n), info, par, cu.info_bits(cu.SEED, 0, B, info.size))
    x.setflags(write=False)
    cls = None
    if name != "D":
        cls = np.zeros(g.n, np.uint8)
        cls[:Z] = rr.PUNCT  # block column 0
    return dict(csr=tuple(np.ascontiguousarray(a, np.int32) for a in g.csr), layer=g.layer_schedule(), n=g.n, cls=cls,
                x=x, quant=cu.QUANT if name != "D" else QUANT_D)


def rows_of(csr, layer, cls, x, llr0, quant, iters, early_stop, known_llr=rr.KNOWN_LLR):
    """(rows int64 [B][iters + 1], its [B], ties) of the words x on the all-zero stream llr0 float32
    [B, n]; ties: how often a counted posterior is 0 where the codeword bit is 1, over iterations
    1 .. iters (the positions the all-zero shortcut would count as correct)."""
    x = np.asarray(x, np.uint8)
    cls = np.zeros(x.shape[1], np.uint8) if cls is None else np.asarray(cls)
    cnt = rr.default_count(cls).astype(bool)
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
def rows(name, p, early_stop, iters=cu.ITERS):
    """rows_of a case on the oracle's BSC stream of crossover probability p (exact against the device)."""
    c = case(name)
    llr0 = oracle.channel(oracle.CH_BSC, p, cu.SEED, 0, c["n"], B)
    out = rows_of(c["csr"], c["layer"], c["cls"], c["x"], llr0, c["quant"], iters, early_stop)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


def counters(name, p, early_stop, X=-1, stop=0, iters=cu.ITERS):
    """The counter vector [trials, frame errors, bit errors, iterations | curve] of one batch."""
    r, its, _ = rows(name, p, early_stop, iters)
    return layered_q_ref.mc_counters(np.asarray(r), np.asarray(its), X, stop)


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


def plane_bytes(n):
    """One bit per variable, in whole words."""
    return 4 * ((n + 31) // 32)
