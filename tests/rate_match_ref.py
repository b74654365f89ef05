"""Numpy restatement of rate matching (include/ldpc_mi355x.h, "Rate matching"): the packed description,
the three channel rules, the per-trial count rows, and the host chain of tests/test_gpu_rate_match.py
built on tests/codeword_util.py.  Nothing here touches the device.
"""
import functools

import numpy as np

from tests import codeword_util as cu, encode_ref, encode_util as eu

TX, PUNCT, KNOWN = 0, 1, 2
KNOWN_LLR = 1024.0


def default_count(cls):
    return (np.asarray(cls) != KNOWN).astype(np.uint8)


def pack(cls, count=None):
    """(packed uint8 [4 ceil(n / 4)], [n, n_tx, n_punct, n_known, n_count]): byte v = cls | count << 2,
    the padding bytes PUNCT and uncounted."""
    cls = np.asarray(cls, np.uint8)
    cnt = default_count(cls) if count is None else np.asarray(count, np.uint8)
    n = cls.size
    packed = np.full(4 * ((n + 3) // 4), PUNCT, np.uint8)
    packed[:n] = cls | cnt << 2
    return packed, [n, int((cls == TX).sum()), int((cls == PUNCT).sum()), int((cls == KNOWN).sum()), int(cnt.sum())]


def apply_rules(out, cls, x, bec, known_llr=KNOWN_LLR):
    """The output of ldpc_channel_cw_dev [B, n] under a description: transmitted positions as they are,
    punctured ones 2 (BEC) / +0.0, known ones x (BEC) / x ? -known_llr : +known_llr."""
    cls = np.asarray(cls)
    out = np.array(out, copy=True)
    x = np.zeros(out.shape, np.uint8) if x is None else np.asarray(x)
    p, k = cls == PUNCT, cls == KNOWN
    if bec:
        out[:, p] = 2
        out[:, k] = x[:, k]
    else:
        out[:, p] = np.float32(0.0)
        out[:, k] = np.where(x[:, k] == 1, np.float32(-known_llr), np.float32(known_llr))
    return out


def rows(cls, count, x, chan, dec, chan_kind, iters):
    """Per-trial rows [B][iters + 1]: row[0] channel errors over class TX and count = 1, row[iters]
    final errors over count = 1, zeros between.  chan_kind 0: BEC words (erased = 2) in chan and dec,
    1: LLRs, 2: received bits."""
    cls = np.asarray(cls)
    cnt = (default_count(cls) if count is None else np.asarray(count)).astype(bool)
    x = np.zeros(np.shape(chan), np.uint8) if x is None else np.asarray(x) & 1
    if chan_kind == 0:
        ce, fe = np.asarray(chan) == 2, np.asarray(dec) == 2
    else:
        y = (np.asarray(chan) < 0).astype(np.uint8) if chan_kind == 1 else np.asarray(chan) & 1
        ce, fe = y != x, (np.asarray(dec) & 1) != x
    out = np.zeros((x.shape[0], iters + 1), np.int64)
    out[:, 0] = (ce & (cnt & (cls == TX))[None, :]).sum(axis=1)
    out[:, iters] = (fe & cnt[None, :]).sum(axis=1)  # iters == 0: the one entry is the final count
    return out


# ------------------------------------------------------------------ the host chain
@functools.lru_cache(maxsize=None)
def description(name, punctured=True):
    """(shortened, punctured) of the named graph: rng = PCG64(2026), 40 shortened positions drawn from
    the encoder's information positions, then 60 punctured of the rest (n = 96: 6 and 8)."""
    n = eu.graph(name)[2]
    ns, np_ = (40, 60) if n == 1000 else (6, 8)
    info_pos = eu.description(name)[1]
    rng = np.random.Generator(np.random.PCG64(2026))
    short = np.sort(rng.choice(info_pos, ns, replace=False))
    rest = np.setdiff1d(np.arange(n), short)
    punct = np.sort(rng.choice(rest, np_, replace=False)) if punctured else np.zeros(0, np.int64)
    return short, punct


def classes(name, punctured=True):
    short, punct = description(name, punctured)
    cls = np.zeros(eu.graph(name)[2], np.uint8)
    cls[punct] = PUNCT
    cls[short] = KNOWN
    return cls


@functools.lru_cache(maxsize=None)
def codewords(name, B, punctured=True):
    """The words of trials 0 .. B - 1 under cu.SEED with the information bits at shortened positions
    zeroed before encoding, read-only."""
    _, info_pos, par_pos, _ = eu.description(name)
    u = cu.info_bits(cu.SEED, 0, B, info_pos.size)
    u[:, np.isin(info_pos, description(name, punctured)[0])] = 0
    x = encode_ref.solve(eu.H(name), info_pos, par_pos, u)
    x.setflags(write=False)
    return x


def chain_llr(name, x, llr_cw, decoder, alpha=1.0, punctured=True):
    """(rows, its, hard) of the words x whose ldpc_channel_cw_dev LLRs are llr_cw: the rules, the
    reference decode of tests/codeword_util.py, the counts under the default mask."""
    cls = classes(name, punctured)
    llr = apply_rules(llr_cw, cls, x, False)
    hard, its = cu.decode(name, llr, decoder, alpha)
    return rows(cls, None, x, llr, hard, 1, cu.ITERS), its, hard


@functools.lru_cache(maxsize=None)
def chain(name, param, B, decoder, alpha=1.0, mode="random", punctured=True):
    """chain_llr on the oracle's BSC stream (exact against the device)."""
    n = eu.graph(name)[2]
    x = codewords(name, B, punctured) if mode == "random" else np.zeros((B, n), np.uint8)
    llr = cu.channel(name, "bsc", param, B, "zero")
    return chain_llr(name, x, np.where(x == 1, -llr, llr).astype(np.float32), decoder, alpha, punctured)
