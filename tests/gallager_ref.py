"""Gallager's hard-decision algorithm A/B on the BSC as include/ldpc_mi355x.h defines it ("Gallager
A/B"), twice: decode_word, a sequential per-slot form in plain integers that follows the text line by
line, and decode, a vectorised numpy form over a batch (what the GPU tests compare with).
tests/test_gallager_ref.py holds the two to each other.

Graph: CSR slot form (check_ptr, check_var, var_ptr, var_slot), taken slot by slot -- a check that
holds a variable twice has two slots.  One bit per edge and direction; b is the flip threshold:

    b_d = d - 1 (b = 0, Gallager A) or min(b, d - 1) (b >= 1, Gallager B); a degree-1 variable sends y_v
    m_vc(e) = y_v
    iteration t = 1 .. max_iters:
      check c:    m_cv(e_j) = XOR_{k != j} m_vc(e_k)
      variable v: dis_j = m_cv(e_j) ^ y_v, D = sum_j dis_j
                  x_v = y_v ^ [2 D > d + 1]
                  m_vc(e_j) = y_v ^ [D - dis_j >= b_d]        (d >= 2)
      early stop: x satisfies every check -> stop, its = t
    hard = x of the last iteration run (max_iters = 0: hard = y, its = 0)
"""
import numpy as np


def flip_threshold(d, b):
    """b_d of a variable of degree d (d >= 2)."""
    return d - 1 if b == 0 else min(b, d - 1)


def decode_word(csr, y, max_iters, b, early_stop):
    """One word, slot by slot in Python integers.  Returns (hard list, its, curve list): curve[t] =
    weight of x after iteration t (curve[0] = weight of y), the tail repeating the last count."""
    cptr, cvar, vptr, vslot = [[int(x) for x in a] for a in csr]
    n, m = len(vptr) - 1, len(cptr) - 1
    y = [int(v) & 1 for v in y]
    msg = [y[cvar[s]] for s in range(cptr[m])]  # v -> c, then c -> v, in place
    x = list(y)
    curve = [sum(y)]
    its = 0
    for t in range(1, max_iters + 1):
        for c in range(m):
            total = 0
            for s in range(cptr[c], cptr[c + 1]):
                total ^= msg[s]
            for s in range(cptr[c], cptr[c + 1]):
                msg[s] ^= total
        for v in range(n):
            slots = vslot[vptr[v]:vptr[v + 1]]
            d = len(slots)
            dis = [msg[s] ^ y[v] for s in slots]
            D = sum(dis)
            x[v] = y[v] ^ int(2 * D > d + 1)
            for j, s in enumerate(slots):
                msg[s] = y[v] ^ int(D - dis[j] >= flip_threshold(d, b)) if d >= 2 else y[v]
        its = t
        curve.append(sum(x))
        if early_stop:
            ok = True
            for c in range(m):
                par = 0
                for s in range(cptr[c], cptr[c + 1]):
                    par ^= x[cvar[s]]
                ok = ok and par == 0
            if ok:
                break
    curve += [curve[-1]] * (max_iters + 1 - len(curve))
    return x, its, curve


def _segment_sum(a, ptr):
    """Row-wise sums of a[:, ptr[i]:ptr[i+1]] (empty segments give 0)."""
    cs = np.concatenate([np.zeros((a.shape[0], 1), np.int64), np.cumsum(a, axis=1, dtype=np.int64)], axis=1)
    return cs[:, ptr[1:]] - cs[:, ptr[:-1]]


def decode(csr, Y, max_iters, b, early_stop):
    """A batch Y [B, n] (bit 0 of each entry is read).  Returns (hard uint8 [B, n], its int64 [B],
    curve int64 [B, max_iters + 1])."""
    cptr, cvar, vptr, vslot = [np.asarray(a, np.int64) for a in csr]
    n, m = vptr.size - 1, cptr.size - 1
    Y = (np.atleast_2d(np.asarray(Y)).astype(np.int64) & 1).astype(np.int64)
    B = Y.shape[0]
    cdeg, vdeg = np.diff(cptr), np.diff(vptr)
    slot_chk = np.repeat(np.arange(m), cdeg)
    edge_var = np.repeat(np.arange(n), vdeg)
    bd = np.where(b == 0, vdeg - 1, np.minimum(b, vdeg - 1))
    hard = Y.copy()
    its = np.zeros(B, np.int64)
    curve = np.zeros((B, max_iters + 1), np.int64)
    curve[:, 0] = Y.sum(axis=1)
    act = np.arange(B)  # rows still decoding
    y = Y
    M = y[:, cvar]
    for t in range(1, max_iters + 1):
        if not act.size:
            break
        M ^= (_segment_sum(M, cptr) & 1)[:, slot_chk]
        mcv = M[:, vslot]                      # in variable-edge order
        dis = mcv ^ y[:, edge_var]
        D = _segment_sum(dis, vptr)
        x = y ^ (2 * D > vdeg + 1)
        flip = ((D[:, edge_var] - dis) >= bd[edge_var]) & (vdeg[edge_var] >= 2)
        M[:, vslot] = y[:, edge_var] ^ flip
        hard[act] = x
        its[act] = t
        curve[act, t:] = x.sum(axis=1)[:, None]
        if early_stop:
            go = (_segment_sum(x[:, cvar], cptr) & 1).any(axis=1)
            act, y, M = act[go], y[go], M[go]
    return hard.astype(np.uint8), its, curve


def mc_counters(curve, its, X=-1, stop=0):
    """The sequential trial loop's counters [trials, frame errors, bit errors, iterations | curve]
    over per-trial curves in trial order (expurgation X, stop at `stop` frame errors; 0: none)."""
    from tests.layered_ref import mc_counters as f
    return f(np.asarray(curve, np.int64), np.asarray(its, np.int64), X, stop)
