"""The host side of tests/test_gpu_mc_codewords.py: the chain information bits (the oracle's Philox)
-> tests/encode_ref.py -> the oracle's channel reflected -> a reference decode -> counts against the
codeword, for the trials of one batch.  Nothing here touches the device.
"""
import functools

import numpy as np

from oracle import oracle
from tests import encode_ref, encode_util as eu, gallager_ref, layered_q_ref, layered_ref

SEED, ITERS = 7, 20
M32 = 2 ** 32 - 1
KIND = {"bsc": oracle.CH_BSC, "awgn": oracle.CH_AWGN}
QUANT = (5, 7, 2.0, 8, 1)  # bits, post_bits, scale, norm8, offset: one of the two headline sets


def info_bits(seed, first, B, K):
    """Bit j of trial t: bit j & 31 of word (j >> 5) & 3 of Philox {j >> 7, 1, t_lo, t_hi}, key {seed_lo, seed_hi}."""
    out = np.zeros((B, K), np.uint8)
    key = [seed & M32, seed >> 32]
    for b in range(B):
        t = first + b
        for blk in range((K + 127) // 128):
            w = oracle.philox([blk, 1, t & M32, t >> 32], key)
            bits = (w[:, None] >> np.arange(32, dtype=np.uint32)[None, :] & 1).astype(np.uint8).ravel()
            j0 = 128 * blk
            out[b, j0:min(K, j0 + 128)] = bits[:min(K, j0 + 128) - j0]
    return out


@functools.lru_cache(maxsize=None)
def csr(name):
    from tests import graph_util
    cptr, cvar, n = eu.graph(name)
    return tuple(np.ascontiguousarray(a, np.int32) for a in graph_util.csr_from_checks(cptr, cvar, n))


@functools.lru_cache(maxsize=None)
def codewords(name, B):
    """The transmitted words uint8 [B, n] of trials 0 .. B - 1 under SEED, read-only."""
    rank, info, par, _ = eu.description(name)
    x = encode_ref.solve(eu.H(name), info, par, info_bits(SEED, 0, B, info.size))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def channel(name, kind, param, B, mode):
    """LLRs float32 [B, n] of trials 0 .. B - 1: the all-zero stream (mode "zero") or its reflection
    where the codeword bit is 1 (mode "random"), read-only."""
    n = eu.graph(name)[2]
    llr = oracle.channel(KIND[kind], param, SEED, 0, n, B)
    if mode == "random":
        llr = np.where(codewords(name, B) == 1, -llr, llr).astype(np.float32)
    llr.setflags(write=False)
    return llr


def layers(name):
    return eu.tanner(name).layer_schedule()


def decode(name, llr, decoder, alpha=1.0):
    """(hard, its) of the reference decode with early stop: "minsum" (the oracle's flooding min-sum),
    "gallager" (A, on the bits llr < 0), "layered" (fp32 min-sum), "layered_q" (QUANT)."""
    c = csr(name)
    if decoder == "minsum":
        _, hard, its = oracle.bp_decode_batch(c, llr, ITERS, 1, alpha=alpha, early_stop=True)
    elif decoder == "gallager":
        hard, its, _ = gallager_ref.decode(c, (llr < 0).astype(np.uint8), ITERS, 0, True)
    elif decoder == "layered":
        _, hard, its, _ = layered_ref.decode(c, layers(name), llr, ITERS, 1, alpha, True)
    else:
        assert decoder == "layered_q"
        hard, its = layered_q_ref.decode(c, layers(name), llr, ITERS, *QUANT, early_stop=True)[1:3]
    return np.asarray(hard, np.uint8), np.asarray(its, np.int64)


def curves(x, llr, hard):
    """Per-trial rows [B][ITERS + 1] of the codeword mode: the two ends counted against x, zeros between."""
    curve = np.zeros((x.shape[0], ITERS + 1), np.int64)
    curve[:, 0] = ((llr < 0).astype(np.uint8) != x).sum(axis=1)
    curve[:, -1] = (hard != x).sum(axis=1)
    return curve


def chain_llr(name, x, llr, decoder, alpha=1.0):
    """(curve [B][ITERS + 1], its [B]) of the codewords x received as llr: decode, count against x."""
    hard, its = decode(name, llr, decoder, alpha)
    return curves(x, llr, hard), its


@functools.lru_cache(maxsize=None)
def chain(name, kind, param, B, decoder, alpha=1.0, mode="random"):
    """chain_llr of the host chain; mode "zero": the all-zero shortcut's.  Exact against the device on
    the BSC, whose stream the oracle restates bit for bit; the oracle's BI-AWGN values are Box-Muller
    in the host's libm and differ from the device's in the last place, so an AWGN chain
    takes the device's own all-zero stream through chain_llr."""
    x = codewords(name, B) if mode == "random" else np.zeros((B, eu.graph(name)[2]), np.uint8)
    return chain_llr(name, x, channel(name, kind, param, B, mode), decoder, alpha)


def ends(counters):
    """Counters [0..3] and the two curve ends of a counter vector."""
    c = np.asarray(counters, np.int64)
    return c[[0, 1, 2, 3, 4, -1]]


def zero_posteriors(name, kind, param, B, alpha):
    """How many posteriors of the all-zero min-sum decode are exactly zero at iterations 1 .. ITERS."""
    llr = channel(name, kind, param, B, "zero")
    return sum(int((oracle.bp_decode_batch(csr(name), llr, t, 1, alpha=alpha, early_stop=False)[0] == 0).sum())
               for t in range(1, ITERS + 1))
