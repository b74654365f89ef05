"""Reference of the fixed-point layered min-sum, the contract of ldpc_bp_layered_q_decode_batch_dev
(include/ldpc_mi355x.h), in numpy and in the per-edge R form, as layered_ref.decode: a sequential
sweep over the checks sorted by (layer, check id), vectorised over the frames of a batch.

    Q = 2^(bits-1) - 1, Pmax = 2^(post_bits-1) - 1
    c[v] = rint_half_even(clamp(float32(llr[v]) * float32(scale), -Q, Q))   (NaN -> 0)
    P = c, R = 0
    iteration t = 1..max_iters, each check, slots e_j, variables v_j:
        x_j = P[v_j] - R[e_j];  a_j = min(|x_j|, Q);  s_j = x_j < 0
        m1 = min a, i1 = first index reaching it, m2 = min over j != i1 (degree 1: Q)
        f(m) = max(((m * norm8) >> 3) - offset, 0)
        |r_j| = f(m2) if j == i1 else f(m1);  r_j < 0 iff (XOR s) ^ s_j and |r_j| > 0
        P[v_j] = clamp(x_j + r_j, -Pmax, Pmax);  R[e_j] = r_j
    hard = P < 0;  early stop: hard satisfies every check -> stop, its = t

Every value after the quantiser is an integer (int32 here), so a decoder either equals this bit
for bit or is wrong.
"""
import numpy as np

from tests.layered_ref import _steps, mc_counters  # noqa: F401  (mc_counters: the Monte-Carlo counters)


def q_of(bits):
    return (1 << (bits - 1)) - 1


def quantise(llr, scale, Q):
    """The channel quantiser on float32 [B, n]: int32 values in [-Q, Q]."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.asarray(llr, np.float32) * np.float32(scale)
    t = np.where(np.isnan(t), np.float32(0), t)
    return np.rint(np.clip(t, np.float32(-Q), np.float32(Q))).astype(np.int32)


def f_mag(mag, norm8, offset):
    return np.maximum(((mag * norm8) >> 3) - offset, 0)


def check_update(x, Q, norm8, offset):
    """The check rule on integer x [B, d]: r [B, d] and the record fields (f(m1), f(m2), i1)."""
    rows = np.arange(x.shape[0])
    a = np.minimum(np.abs(x), Q)
    s = x < 0
    par = np.bitwise_xor.reduce(s, axis=1)
    i1 = np.argmin(a, axis=1)  # the first index reaching the minimum
    m1 = a[rows, i1]
    rest = a.copy()
    rest[rows, i1] = Q  # degree 1: m2 = Q (every a_j <= Q)
    m2 = rest.min(axis=1)
    f1, f2 = f_mag(m1, norm8, offset), f_mag(m2, norm8, offset)
    first = np.arange(x.shape[1])[None, :] == i1[:, None]
    mag = np.where(first, f2[:, None], f1[:, None])
    neg = (par[:, None] ^ s) & (mag > 0)
    return np.where(neg, -mag, mag).astype(np.int32), (f1, f2, i1)


def decode(csr, layer, llr, max_iters, bits, post_bits, scale, norm8=6, offset=0, early_stop=False, at=(),
           by_layer=True):
    """csr: (check_ptr, check_var, ...); layer: int[m] the layer of every check; llr float32 [B, n].
    Returns (post int8 [B, n], hard uint8 [B, n], its int32 [B], curve int64 [B, max_iters + 1],
    sat): curve[:, 0] = quantised channel values < 0, curve[:, t] = posteriors < 0 after iteration
    t, repeated after a stop; sat = the number of saturation events so far (an |x_j| > Q, or a
    posterior that the clamp changed), over all frames.  at: as layered_ref.decode -- the result
    is then the dict {t: tuple} over `at` and max_iters."""
    cptr, cvar = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int64)
    m = cptr.size - 1
    layer = np.asarray(layer)
    assert layer.shape == (m,) and np.all(np.diff(cptr) > 0)
    steps = _steps(cptr, cvar, layer, by_layer)
    Q, Pmax = q_of(bits), q_of(post_bits)
    llr = np.ascontiguousarray(np.atleast_2d(llr), np.float32)
    B = llr.shape[0]
    P = quantise(llr, scale, Q)
    R = np.zeros((B, cvar.size), np.int32)
    its = np.full(B, max_iters, np.int32)
    curve = np.zeros((B, max_iters + 1), np.int64)
    curve[:, 0] = (P < 0).sum(axis=1)
    active = np.ones(B, bool)
    sat = 0
    out = {}

    def result(t):
        c = curve[:, :t + 1].copy()
        return P.astype(np.int8), (P < 0).astype(np.uint8), np.where(active, t, its).astype(np.int32), c, sat

    if 0 in at or max_iters == 0:
        out[0] = result(0)
    for t in range(1, max_iters + 1):
        idx = np.nonzero(active)[0]
        if idx.size:
            Pa, Ra = P[idx], R[idx]
            for V, S in steps:
                x = Pa[:, V] - Ra[:, S]
                flat = x.reshape(-1, x.shape[2])
                r = check_update(flat, Q, norm8, offset)[0].reshape(x.shape)
                new = x + r
                clamped = np.clip(new, -Pmax, Pmax)
                sat += int((np.abs(x) > Q).sum()) + int((clamped != new).sum())
                Pa[:, V] = clamped
                Ra[:, S] = r
            P[idx], R[idx] = Pa, Ra
            if early_stop:
                par = np.bitwise_xor.reduceat(Pa[:, cvar] < 0, cptr[:-1], axis=1)
                done = ~par.any(axis=1)
                its[idx[done]] = t
                active[idx[done]] = False
        curve[:, t] = (P < 0).sum(axis=1)
        if t in at or t == max_iters:
            out[t] = result(t)
    return out if at else out[max_iters]
