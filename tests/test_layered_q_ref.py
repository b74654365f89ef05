"""The fixed-point layered min-sum's reference (tests/layered_q_ref.py) held to itself, to the fp32
layered reference and to a hand-worked check; and the parameter rules (no device needed).

* Record form: a second sweep that keeps, per check, only the record (f(m1), f(m2), i1, sign bits)
  and rebuilds R from it equals the per-edge sweep bit for bit.
* On small integer LLRs with wide formats nothing saturates, and the integers equal
  layered_ref.decode's fp32 min-sum (alpha = 1) exactly.
* A degree-3 check by hand: a tie of the minima, a zero input, the offset driving a magnitude to
  0, posteriors clamping.
* decoder.Quant, ldpc_quant_check and ldpc_debug_layer_q_plan refuse what the contract forbids.
"""
import ctypes as ct

import numpy as np
import pytest

from tests import layered_q_ref, layered_ref
from tests.layered_util import graph_csr, layers
from tests.layered_q_util import layer_q_plans


def _awgn(n, frames, sigma, seed):
    rng = np.random.default_rng(seed)
    return ((2.0 / sigma ** 2) * (1.0 + sigma * rng.standard_normal((frames, n)))).astype(np.float32)


# ------------------------------------------------------------------ record form
def _decode_records(csr, layer, llr, iters, bits, post_bits, scale, norm8, offset):
    """The sweep a decoder with compressed records runs: per check f(m1), f(m2), i1 and one sign
    bit per edge; R_j is rebuilt from them, never stored."""
    cptr, cvar = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int64)
    m = cptr.size - 1
    Q, Pmax = layered_q_ref.q_of(bits), layered_q_ref.q_of(post_bits)
    P = layered_q_ref.quantise(llr, scale, Q)
    B = P.shape[0]
    f1, f2, i1 = (np.zeros((B, m), np.int64) for _ in range(3))
    sign = np.zeros((B, m), np.uint32)
    order = np.lexsort((np.arange(m), layer))
    for _ in range(iters):
        for c in order:
            v = cvar[cptr[c]:cptr[c + 1]]
            j = np.arange(v.size)
            mag = np.where(j[None, :] == i1[:, c, None], f2[:, c, None], f1[:, c, None])
            R = np.where((sign[:, c, None] >> j[None, :].astype(np.uint32)) & 1, -mag, mag)
            x = P[:, v] - R
            r, (g1, g2, k1) = layered_q_ref.check_update(x, Q, norm8, offset)
            P[:, v] = np.clip(x + r, -Pmax, Pmax)
            f1[:, c], f2[:, c], i1[:, c] = g1, g2, k1
            sign[:, c] = ((r < 0).astype(np.uint32) << j[None, :].astype(np.uint32)).sum(axis=1, dtype=np.uint32)
            assert g1.max() <= 63 and g2.max() <= 63 and k1.max() < 32  # the fields of the record
    return P.astype(np.int8)


@pytest.mark.parametrize("params", [(6, 8, 2.0, 6, 0), (4, 6, 0.5, 8, 1), (6, 6, 2.0, 6, 0)])
@pytest.mark.parametrize("name", ["r36_600", "mixB"])
def test_record_form_equals_per_edge_form(name, params):
    csr, layer = graph_csr(name), layers(name)[1]
    llr = _awgn(csr[2].size - 1, 8, 0.8, 4)
    want = layered_q_ref.decode(csr, layer, llr, 5, *params)
    np.testing.assert_array_equal(_decode_records(csr, layer, llr, 5, *params), want[0])
    # and the per-check sweep equals the per-layer one
    slow = layered_q_ref.decode(csr, layer, llr, 5, *params, by_layer=False)
    for a, b in zip(want, slow):
        np.testing.assert_array_equal(a, b)


# --------------------------------------------------- tie to the fp32 reference
@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("name", ["r36_600", "r58_320"])
def test_integer_llrs_equal_the_fp32_layered_min_sum(name, early_stop):
    csr, layer = graph_csr(name), layers(name)[1]
    llr = np.random.default_rng(17).integers(-2, 6, size=(8, csr[2].size - 1)).astype(np.float32)
    got = layered_q_ref.decode(csr, layer, llr, 5, 7, 8, 1.0, 8, 0, early_stop, at=(1, 2, 3))
    want = layered_ref.decode(csr, layer, llr, 5, 1, 1.0, early_stop, at=(1, 2, 3))
    for t in (1, 2, 3, 5):
        post, hard, its, curve, sat = got[t]
        assert sat == 0, (name, t)
        np.testing.assert_array_equal(post.astype(np.float32), want[t][0])
        np.testing.assert_array_equal(hard, want[t][1])
        np.testing.assert_array_equal(its, want[t][2])
        np.testing.assert_array_equal(curve, want[t][3])
        assert np.abs(post.astype(np.int32)).max() < 63


# ------------------------------------------------------- a degree-3 check by hand
ONE_CHECK = (np.array([0, 3], np.int32), np.array([0, 1, 2], np.int32), np.array([0, 1, 2, 3], np.int32),
             np.array([0, 1, 2], np.int32))


def test_hand_worked_degree_3_check():
    upd = layered_q_ref.check_update
    # a tie of the minima: the FIRST index takes f(m2) = f(m1); Q = 7, f(m) = m - 1
    r, (f1, f2, i1) = upd(np.array([[3, -3, 5]]), 7, 8, 1)
    assert (f1[0], f2[0], i1[0]) == (2, 2, 0) and r.tolist() == [[-2, 2, -2]]
    # a zero input counts as positive and is the minimum; the offset drives f(0) to 0, and a zero
    # message is never negative: only the first index, which takes f(m2) = f(4) = 3, hears anything
    r, (f1, f2, i1) = upd(np.array([[0, -4, 6]]), 7, 8, 1)
    assert (f1[0], f2[0], i1[0]) == (0, 3, 0) and r.tolist() == [[-3, 0, 0]]
    # normalisation alone: (1 * 6) >> 3 = 0, (2 * 6) >> 3 = 1
    r, (f1, f2, i1) = upd(np.array([[1, -2, 7]]), 7, 6, 0)
    assert (f1[0], f2[0], i1[0]) == (0, 1, 0) and r.tolist() == [[-1, 0, 0]]
    # magnitudes are taken from min(|x|, Q): x = 12 enters as 7
    r, (f1, f2, i1) = upd(np.array([[12, 9, -8]]), 7, 8, 0)
    assert (f1[0], f2[0], i1[0]) == (7, 7, 0) and r.tolist() == [[-7, -7, 7]]
    # degree 1: m2 = Q, and the parity of the others (none) is even
    r, (f1, f2, i1) = upd(np.array([[-2]]), 7, 8, 0)
    assert (f1[0], f2[0], i1[0]) == (2, 7, 0) and r.tolist() == [[7]]
    # posteriors clamping, 4-bit messages and 4-bit posteriors (Pmax = 7): c = (7, 7, 6);
    # iteration 1: x = c, r = (6, 6, 7), P = clamp(13, 13, 13) = (7, 7, 7), three clamps;
    # iteration 2: x = P - R = (1, 1, 0), r = (0, 0, 1), P = (1, 1, 1) -- what the clamp lost
    llr = np.array([[7.2, 30.0, 5.5]], np.float32)  # 5.5 rounds to the even 6
    out = layered_q_ref.decode(ONE_CHECK, np.zeros(1, np.int64), llr, 2, 4, 4, 1.0, 8, 0, at=(0, 1))
    assert out[0][0].tolist() == [[7, 7, 6]] and out[0][4] == 0
    assert out[1][0].tolist() == [[7, 7, 7]] and out[1][4] == 3
    assert out[2][0].tolist() == [[1, 1, 1]] and out[2][4] == 3
    # 5-bit posteriors (Pmax = 15) keep 13, and the decoder sits at its fixed point
    out = layered_q_ref.decode(ONE_CHECK, np.zeros(1, np.int64), llr, 2, 4, 5, 1.0, 8, 0, at=(1,))
    assert out[1][0].tolist() == [[13, 13, 13]] and out[2][0].tolist() == [[13, 13, 13]] and out[2][4] == 0


def test_quantiser():
    q = layered_q_ref.quantise
    llr = np.array([[0.25, 0.75, 1.25, -0.25, -0.75, np.nan, np.inf, -np.inf, -0.0, 1e-40, 1e38, -1e38]], np.float32)
    assert q(llr, 2.0, 31).tolist() == [[0, 2, 2, 0, -2, 0, 31, -31, 0, 0, 31, -31]]  # halves to even


# ---------------------------------------------------------- parameter validation
VALID = [(2, 2, 0.25, 8, 0), (7, 8, 4.0, 6, 0), (4, 6, 0.5, 8, 1), (6, 6, 2.0, 1, 31), (7, 7, 1e-3, 8, 63)]
INVALID = [(1, 4, 1.0, 6, 0), (8, 8, 1.0, 6, 0), (6, 5, 1.0, 6, 0), (6, 9, 1.0, 6, 0), (6, 8, 1.0, 0, 0),
           (6, 8, 1.0, 9, 0), (6, 8, 1.0, 6, -1), (6, 8, 1.0, 6, 32), (2, 2, 1.0, 8, 2), (6, 8, 0.0, 6, 0),
           (6, 8, -1.0, 6, 0), (6, 8, float("inf"), 6, 0), (6, 8, float("nan"), 6, 0)]


def _native_check(p):
    from iib_project_ldpc_codes_amd import _native
    q = _native.Quant(p[2], p[0], p[1], p[3], p[4])
    return _native.lib().ldpc_quant_check(ct.addressof(q))


def test_parameter_rules():
    from iib_project_ldpc_codes_amd import _native
    from iib_project_ldpc_codes_amd.decoder import Quant
    for p in VALID:
        q = Quant(*p)
        assert (q.Q, q.Pmax) == ((1 << (p[0] - 1)) - 1, (1 << (p[1] - 1)) - 1)
        assert q == Quant(*p) and q.as_dict() == dict(zip(Quant.FIELDS, (p[0], p[1], float(np.float32(p[2])), p[3], p[4])))
        assert _native_check(p) == 0, p
    assert Quant(5, 6, 1.5).as_dict() == {"bits": 5, "post_bits": 6, "scale": 1.5, "norm8": 6, "offset": 0}
    for p in INVALID:
        with pytest.raises(ValueError):
            Quant(*p)
        assert _native_check(p) == _native.LDPC_EINVAL, p
    with pytest.raises(ValueError):
        Quant(5.5, 6, 1.0)
    with pytest.raises(ValueError):
        Quant(6, 8, 1e-60)  # 0 as a float32
    assert _native.lib().ldpc_quant_check(None) == _native.LDPC_EINVAL


def test_plan_entry_refusals():
    from iib_project_ldpc_codes_amd import _native
    csr = graph_csr("r36_600")
    assert layer_q_plans(csr, [(1, 0, 0, 1, 20, 24)], cus=0, rc_only=True) == _native.LDPC_EINVAL
    assert layer_q_plans(csr, [(1, 0, 0, 1, 20, -1)], rc_only=True) == _native.LDPC_EINVAL
    assert layer_q_plans(csr, [(1, 0, 0, 1, -1, 24)], rc_only=True) == _native.LDPC_EINVAL
    # a check that holds a variable twice has no layer schedule
    twice = (np.array([0, 3], np.int32), np.array([0, 1, 1], np.int32), np.array([0, 1, 3], np.int32),
             np.array([0, 1, 2], np.int32))
    assert layer_q_plans(twice, [(1, 0, 0, 1, 20, 24)], rc_only=True) == _native.LDPC_EUNSUP
    assert layer_q_plans(csr, []) == []


def test_quant_needs_layered_min_sum():
    """The argument checks come before any device is asked for."""
    from iib_project_ldpc_codes_amd import decoder
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    q = decoder.Quant(6, 8, 2.0)
    llr = np.zeros((1, 600), np.float32)
    for kw in ({"schedule": "flooding", "algo": "minsum"}, {"schedule": "layered", "algo": "spa"}, {"algo": "minsum"}):
        with pytest.raises(ValueError):
            decoder.bp_decode(None, llr, 5, quant=q, **kw)
        with pytest.raises(ValueError):
            decoder.bp_decode_dev(None, llr, 5, quant=q, **kw)
        with pytest.raises(ValueError):
            MonteCarlo(None, "bsc", 0.07, 20, quant=q, **kw)
    with pytest.raises(ValueError):
        decoder.bp_decode(None, llr, 5, "minsum", schedule="layered", quant=(6, 8, 2.0))
