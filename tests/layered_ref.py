"""Reference of the layered (row-serial) schedule, the contract of ldpc_bp_layered_decode_batch_dev
(include/ldpc_mi355x.h), in numpy: a sequential sweep over the checks sorted by (layer, check id),
vectorised over the frames of a batch (one Python step per check, or per layer and degree).

    P[v] = llr[v] (min-sum: llr[v] + 0.0f)            R[e] = +0
    iteration t = 1..max_iters:
      for each check c in (layer, id) order, slots e_j, variables v_j:
          x_j = P[v_j] - R[e_j];  r = check rule on x;  P[v_j] = x_j + r_j;  R[e_j] = r_j   (fp32)
      hard[v] = P[v] < 0;  early stop: hard satisfies every check -> stop, its = t

The check rules restate oracle.check_update: min-sum in fp32 (bit-exact with oracle algo 1),
sum-product as float64 tanh / atanh with inputs clamped at 23 ln 2 and rounded to fp32 (oracle
algo 0; tests/test_layer_schedule.py holds both to the oracle).
"""
import numpy as np

XMAX = 23 * np.log(2.0)


def check_update_ms(x, alpha):
    """Normalized min-sum on x float32 [B, d]: the first minimum gets the second smallest
    magnitude, every other edge the smallest; signs by parity of (x < 0)."""
    x = np.asarray(x, np.float32)
    rows = np.arange(x.shape[0])
    a = np.abs(x)
    neg = x < 0
    par = np.bitwise_xor.reduce(neg, axis=1)
    i1 = np.argmin(a, axis=1)  # the first minimum, as the oracle's strict a < m1
    m1 = a[rows, i1]
    rest = a.copy()
    rest[rows, i1] = np.inf
    m2 = rest.min(axis=1)
    first = np.arange(x.shape[1])[None, :] == i1[:, None]
    mag = np.float32(alpha) * np.where(first, m2[:, None], m1[:, None]).astype(np.float32)
    return np.where(par[:, None] ^ neg, -mag, mag).astype(np.float32)


def check_update_spa(x):
    """Sum-product on x float32 [B, d] in float64: exclusive products of tanh(x / 2), |x| clamped at
    23 ln 2, by prefix / suffix products in the oracle's order; 2 atanh of them rounded to fp32."""
    t = np.tanh(0.5 * np.clip(np.asarray(x, np.float32).astype(np.float64), -XMAX, XMAX))
    d = t.shape[1]
    pre = np.ones_like(t)
    pre[:, 1:] = np.cumprod(t[:, :-1], axis=1)
    suf = np.ones_like(t)
    suf[:, :d - 1] = np.cumprod(t[:, :0:-1], axis=1)[:, ::-1]
    return (2.0 * np.arctanh(pre * suf)).astype(np.float32)


def _steps(cptr, cvar, layer, by_layer):
    """The sweep's steps, each (variables [g, d], slots [g, d]) of g checks of one degree d: every
    check alone in (layer, check id) order, or -- by_layer -- the checks of a layer at once, one
    step per degree (the checks of a layer share no variable, so their order within it is free:
    tests/test_layer_schedule.py holds the two sweeps to each other bit for bit)."""
    m = cptr.size - 1
    deg = np.diff(cptr)
    order = np.lexsort((np.arange(m), layer))
    if by_layer:
        groups = [order[(layer[order] == l) & (deg[order] == d)] for l in range(int(layer.max()) + 1)
                  for d in np.unique(deg[layer == l])]
    else:
        groups = [order[i:i + 1] for i in range(m)]
    steps = []
    for g in groups:
        slots = cptr[g][:, None] + np.arange(deg[g[0]])[None, :]
        steps.append((cvar[slots], slots))
    return steps


def decode(csr, layer, llr, max_iters, algo, alpha=1.0, early_stop=False, at=(), by_layer=True):
    """csr: (check_ptr, check_var, ...); layer: int[m] the layer of every check; llr float32 [B, n];
    algo 0 sum-product, 1 min-sum.  Returns (post float32 [B, n], hard uint8 [B, n], its int32 [B],
    curve int64 [B, max_iters + 1]): curve[:, 0] = channel errors, curve[:, t] = posteriors < 0
    after iteration t, repeated after a stop.  at: iteration counts t <= max_iters for which the
    same tuple of a decode with max_iters = t is wanted too (a shorter decode is a prefix of a
    longer one); the result is then the dict {t: tuple} over `at` and max_iters."""
    cptr, cvar = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int64)
    m = cptr.size - 1
    layer = np.asarray(layer)
    assert layer.shape == (m,) and np.all(np.diff(cptr) > 0)
    steps = _steps(cptr, cvar, layer, by_layer)
    llr = np.ascontiguousarray(np.atleast_2d(llr), np.float32)
    B = llr.shape[0]
    P = llr + np.float32(0.0) if algo == 1 else llr.copy()
    R = np.zeros((B, cvar.size), np.float32)
    its = np.full(B, max_iters, np.int32)
    curve = np.zeros((B, max_iters + 1), np.int64)
    curve[:, 0] = (llr < 0).sum(axis=1)
    active = np.ones(B, bool)
    out = {}

    def result(t):
        c = curve[:, :t + 1].copy()
        return P.copy(), (P < 0).astype(np.uint8), np.where(active, t, its).astype(np.int32), c

    if 0 in at or max_iters == 0:
        out[0] = result(0)
    for t in range(1, max_iters + 1):
        idx = np.nonzero(active)[0]
        if idx.size:
            Pa, Ra = P[idx], R[idx]
            for V, S in steps:
                x = Pa[:, V] - Ra[:, S]
                flat = x.reshape(-1, x.shape[2])
                r = (check_update_ms(flat, alpha) if algo == 1 else check_update_spa(flat)).reshape(x.shape)
                Pa[:, V] = x + r
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


def mc_counters(curve, its, expurgation=-1, stop_frame_errors=0):
    """The counters ldpc_mc_batch_dev derives from per-trial curves (csrc/mc_kernels.hip): trial b
    is a frame error when its final count f > expurgation and f != 0; with stop_frame_errors
    only the trials up to and including the one that reaches it count; curve, frame and bit
    errors take the trials with f > expurgation, trials and iterations all counted ones."""
    f = curve[:, -1]
    fe = (f > expurgation) & (f != 0)
    cut = curve.shape[0]
    if stop_frame_errors > 0:
        hit = np.nonzero(np.cumsum(fe) >= stop_frame_errors)[0]
        if hit.size:
            cut = int(hit[0]) + 1
    keep = f[:cut] > expurgation
    out = np.zeros(4 + curve.shape[1], np.int64)
    out[0] = cut
    out[1] = int(fe[:cut].sum())
    out[2] = int(f[:cut][keep].sum())
    out[3] = int(np.asarray(its[:cut], np.int64).sum())
    out[4:] = curve[:cut][keep].sum(axis=0)
    return out
