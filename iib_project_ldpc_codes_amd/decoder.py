"""Batched decoders on the MI355X (device tensors via torch, host arrays via the C ABI).

* ``bec_decode``  -- message_passing.c:7-82 over a batch of words (bit-exact).
* ``bp_decode``   -- flooding sum-product / normalized min-sum (new capability);
                     ``schedule="layered"``: the row-serial schedule of hardware decoders.
* ``bp_ensemble_decode_dev`` -- the same decoders, word b on its own device-sampled graph b.
* ``ml_decode``   -- ML ("optimal") erasure decoding, optimal_decode of
                     parallel_simulator.py:60-129 (GF(2) elimination on the device).
* ``channel``     -- on-device BEC / BSC / BI-AWGN channel outputs (Philox).

Device forms take torch CUDA(HIP) tensors and run asynchronously on the
current torch stream; host forms take numpy arrays and block.
"""
import numpy as np

from . import _native
from ._native import ALGO_MINSUM, ALGO_SPA, CH_AWGN, CH_BEC, CH_BSC  # noqa: F401

ALGOS = {"spa": ALGO_SPA, "sum-product": ALGO_SPA, "minsum": ALGO_MINSUM, "min-sum": ALGO_MINSUM,
         ALGO_SPA: ALGO_SPA, ALGO_MINSUM: ALGO_MINSUM}
CHANNELS = {"bec": CH_BEC, "bsc": CH_BSC, "awgn": CH_AWGN, "biawgn": CH_AWGN,
            CH_BEC: CH_BEC, CH_BSC: CH_BSC, CH_AWGN: CH_AWGN}
SCHEDULES = ("flooding", "layered")


def layer_rule(graph=None):
    """Name of the rule that colours a graph's checks into layers (snapshot.LAYER_RULE); with a
    graph, the rule that gave that graph its layers (a quasi-cyclic code's: "qc/block-row/v1")."""
    if graph is not None and hasattr(graph, "layer_rule"):
        return graph.layer_rule
    return _native.lib().ldpc_layer_rule().decode()


def _schedule(schedule):
    if schedule not in SCHEDULES:
        raise ValueError(f"schedule must be one of {SCHEDULES}, not {schedule!r}")
    return schedule


class Quant:
    """Parameters of the fixed-point layered min-sum (ldpc_quant, include/ldpc_mi355x.h): `bits`-bit
    messages (magnitudes up to Q = 2^(bits-1) - 1), `post_bits`-bit saturating posteriors, channel
    LLRs quantised as rint(clamp(llr * scale, -Q, Q)), check magnitudes f(m) = max(((m * norm8) >> 3)
    - offset, 0).  Valid: 2 <= bits <= 7, bits <= post_bits <= 8, 1 <= norm8 <= 8, 0 <= offset <= Q,
    scale finite and > 0 (ValueError otherwise)."""
    FIELDS = ("bits", "post_bits", "scale", "norm8", "offset")

    def __init__(self, bits, post_bits, scale, norm8=6, offset=0):
        for name, x in (("bits", bits), ("post_bits", post_bits), ("norm8", norm8), ("offset", offset)):
            if isinstance(x, bool) or int(x) != x:
                raise ValueError(f"Quant: {name} must be an integer, not {x!r}")
        self.bits, self.post_bits, self.norm8, self.offset = int(bits), int(post_bits), int(norm8), int(offset)
        self.scale = float(np.float32(scale))
        if not 2 <= self.bits <= 7:
            raise ValueError("Quant: need 2 <= bits <= 7")
        if not self.bits <= self.post_bits <= 8:
            raise ValueError("Quant: need bits <= post_bits <= 8")
        if not 1 <= self.norm8 <= 8:
            raise ValueError("Quant: need 1 <= norm8 <= 8")
        if not 0 <= self.offset <= self.Q:
            raise ValueError("Quant: need 0 <= offset <= Q = 2^(bits-1) - 1")
        if not (np.isfinite(self.scale) and self.scale > 0):
            raise ValueError("Quant: scale must be finite and > 0 (as a float32)")

    @property
    def Q(self):
        return (1 << (self.bits - 1)) - 1

    @property
    def Pmax(self):
        return (1 << (self.post_bits - 1)) - 1

    def as_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def native(self):
        return _native.Quant(self.scale, self.bits, self.post_bits, self.norm8, self.offset)

    def __eq__(self, other):
        return isinstance(other, Quant) and self.as_dict() == other.as_dict()

    def __hash__(self):
        return hash(tuple(self.as_dict().items()))

    def __repr__(self):
        return "Quant(%d, %d, %r, norm8=%d, offset=%d)" % (self.bits, self.post_bits, self.scale, self.norm8, self.offset)


def _quant(quant, schedule, algo):
    """None, or the Quant of a call: it needs the layered schedule and min-sum."""
    if quant is None:
        return None
    if not isinstance(quant, Quant):
        raise ValueError(f"quant must be a decoder.Quant, not {quant!r}")
    if _schedule(schedule) != "layered" or ALGOS[algo] != ALGO_MINSUM:
        raise ValueError('quant needs schedule="layered" and algo="minsum" (the fixed-point layered min-sum)')
    return quant


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _native.LdpcError("device", _native.LDPC_ENODEV, "no HIP device visible to torch")
    return torch


def _stream(stream=None):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


# ----------------------------------------------------------------------- BEC
def bec_decode_dev(graph, words, max_iters, errors=None, its=None, stream=None):
    """words: uint8 [B, n] device tensor (0/1/2), decoded in place.
    errors: int32 [B, max_iters] (accumulated like message_passing.c:73; zeros if None).
    Returns (words, errors, its)."""
    torch = _torch()
    B = words.shape[0]
    if errors is None:
        errors = torch.zeros((B, max_iters), dtype=torch.int32, device=words.device)
    if its is None:
        its = torch.empty((B,), dtype=torch.int32, device=words.device)
    assert words.dtype == torch.uint8 and words.is_contiguous() and words.shape[1] == graph.n
    assert errors.dtype == torch.int32 and errors.is_contiguous() and tuple(errors.shape) == (B, max_iters)
    rc = _native.lib().ldpc_bec_decode_batch_dev(graph.handle(), words.data_ptr(), B, max_iters,
                                                 errors.data_ptr(), its.data_ptr(), _stream(stream))
    _native.check(rc, "ldpc_bec_decode_batch_dev")
    return words, errors, its


def bec_decode(graph, words, max_iters, errors=None):
    """Host form: words uint8/int [B, n] numpy (0/1/2).  Returns (words, errors, its)."""
    w = np.ascontiguousarray(np.atleast_2d(words), dtype=np.uint8).copy()
    B = w.shape[0]
    err = (np.zeros((B, max_iters), np.int32) if errors is None
           else np.ascontiguousarray(errors, dtype=np.int32).reshape(B, max_iters).copy())
    its = np.zeros(B, np.int32)
    if graph.csr is not None:
        torch = _torch()
        tw = torch.from_numpy(w).cuda()
        te = torch.from_numpy(err).cuda()
        _, te, ti = bec_decode_dev(graph, tw, max_iters, te)
        torch.cuda.synchronize()
        return tw.cpu().numpy(), te.cpu().numpy(), ti.cpu().numpy()
    rc = _native.lib().ldpc_bec_decode_batch(graph.variable_lookup.ctypes.data, graph.check_lookup.ctypes.data,
                                             graph.n, graph.k, graph.dv, graph.dc, w.ctypes.data, B, max_iters,
                                             err.ctypes.data, its.ctypes.data)
    _native.check(rc, "ldpc_bec_decode_batch")
    return w, err, its


# ------------------------------------------------------------------------ ML
def ml_decode_dev(graph, words, out=None, unsolved=None, stream=None):
    """words: uint8 [B, n] device tensor (0/1 known, 2 erased).  Returns (out, unsolved):
    decoded words with 2 where the reference's loop gives an unknown up, and the
    number of 2s per word (parallel_simulator.py:60-129, :235)."""
    torch = _torch()
    assert words.dtype == torch.uint8 and words.is_contiguous() and words.shape[1] == graph.n
    B = words.shape[0]
    if out is None:
        out = torch.empty_like(words)
    if unsolved is None:
        unsolved = torch.empty((B,), dtype=torch.int32, device=words.device)
    rc = _native.lib().ldpc_ml_decode_batch_dev(graph.handle(), words.data_ptr(), B, out.data_ptr(),
                                                unsolved.data_ptr(), _stream(stream))
    _native.check(rc, "ldpc_ml_decode_batch_dev")
    return out, unsolved


def ml_decode(graph, words):
    """Host form: words uint8 [B, n] numpy.  Returns (out, unsolved) numpy."""
    w = np.ascontiguousarray(np.atleast_2d(words), dtype=np.uint8)
    B = w.shape[0]
    out = np.zeros_like(w)
    uns = np.zeros(B, np.int32)
    rc = _native.lib().ldpc_ml_decode_batch(graph.handle(), w.ctypes.data, B, out.ctypes.data, uns.ctypes.data)
    _native.check(rc, "ldpc_ml_decode_batch")
    return out, uns


def ml_ensemble_decode_dev(n, dv, dc, check_lookup, words, out=None, unsolved=None, stream=None):
    """Word b decoded on graph b: check_lookup int32 [B, n*dv] device tensor
    (graph.sample_device / ldpc_sample_regular_dev layout)."""
    torch = _torch()
    B = words.shape[0]
    assert check_lookup.dtype == torch.int32 and check_lookup.is_contiguous()
    assert tuple(check_lookup.shape) == (B, n * dv) and words.dtype == torch.uint8 and words.shape[1] == n
    if out is None:
        out = torch.empty_like(words)
    if unsolved is None:
        unsolved = torch.empty((B,), dtype=torch.int32, device=words.device)
    rc = _native.lib().ldpc_ml_ensemble_decode_dev(n, dv, dc, check_lookup.data_ptr(), words.data_ptr(), B,
                                                   out.data_ptr(), unsolved.data_ptr(), _stream(stream))
    _native.check(rc, "ldpc_ml_ensemble_decode_dev")
    return out, unsolved


# ---------------------------------------------------------------------- soft
def bp_decode_dev(graph, llr, max_iters, algo="spa", alpha=1.0, early_stop=False, post=None, hard=None,
                  its=None, stream=None, want_post=True, want_hard=True, schedule="flooding", quant=None):
    """llr: float32 [B, n] device tensor.  Returns (post, hard, its) device tensors.
    schedule: "flooding" (all checks, then all variables) or "layered" (row-serial: every check
    works on the posteriors the checks before it updated, graph.layer_schedule() gives the
    order; about half the iterations of flooding to converge).
    quant: a Quant runs the fixed-point layered min-sum (schedule="layered", algo="minsum"; alpha is
    not read): post is then int8 [B, n], the integer posteriors."""
    quant = _quant(quant, schedule, algo)
    torch = _torch()
    B = llr.shape[0]
    entry = "ldpc_bp_decode_batch_dev" if _schedule(schedule) == "flooding" else "ldpc_bp_layered_decode_batch_dev"
    assert llr.dtype == torch.float32 and llr.is_contiguous() and llr.shape[1] == graph.n
    if post is None and want_post:
        post = torch.empty_like(llr) if quant is None else torch.empty(llr.shape, dtype=torch.int8, device=llr.device)
    if hard is None and want_hard:
        hard = torch.empty(llr.shape, dtype=torch.uint8, device=llr.device)
    if its is None:
        its = torch.empty((B,), dtype=torch.int32, device=llr.device)
    if quant is not None:
        import ctypes as ct
        assert post is None or (post.dtype == torch.int8 and post.is_contiguous() and post.shape == llr.shape)
        q = quant.native()
        entry = "ldpc_bp_layered_q_decode_batch_dev"
        rc = getattr(_native.lib(), entry)(graph.handle(), llr.data_ptr(), B, max_iters, ct.addressof(q),
                                           int(bool(early_stop)), _ptr(post), _ptr(hard), _ptr(its), _stream(stream))
        _native.check(rc, entry)
        return post, hard, its
    rc = getattr(_native.lib(), entry)(graph.handle(), llr.data_ptr(), B, max_iters, ALGOS[algo],
                                       float(alpha), int(bool(early_stop)), _ptr(post), _ptr(hard),
                                       _ptr(its), _stream(stream))
    _native.check(rc, entry)
    return post, hard, its


def bp_decode(graph, llr, max_iters, algo="spa", alpha=1.0, early_stop=False, schedule="flooding", quant=None):
    """Host form: llr float32 [B, n] numpy.  Returns (post, hard, its) numpy (post int8 with a Quant)."""
    quant = _quant(quant, schedule, algo)
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(llr), dtype=np.float32)).cuda()
    post, hard, its = bp_decode_dev(graph, t, max_iters, algo, alpha, early_stop, schedule=schedule, quant=quant)
    torch.cuda.synchronize()
    return post.cpu().numpy(), hard.cpu().numpy(), its.cpu().numpy()


def bp_ensemble_decode_dev(n, dv, dc, check_lookup, variable_lookup, llr, max_iters, algo="spa", alpha=1.0,
                           early_stop=False, post=None, hard=None, its=None, stream=None, want_post=True,
                           want_hard=True):
    """Word b decoded on graph b: check_lookup / variable_lookup int32 [B, n*dv] device tensors
    as graph.sample_device / ldpc_sample_regular_dev write them (simple graphs; only read), llr
    float32 [B, n].  Returns (post, hard, its) device tensors."""
    torch = _torch()
    B = llr.shape[0]
    assert llr.dtype == torch.float32 and llr.is_contiguous() and llr.shape[1] == n
    for t in (check_lookup, variable_lookup):
        assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (B, n * dv)
    if post is None and want_post:
        post = torch.empty_like(llr)
    if hard is None and want_hard:
        hard = torch.empty(llr.shape, dtype=torch.uint8, device=llr.device)
    if its is None:
        its = torch.empty((B,), dtype=torch.int32, device=llr.device)
    rc = _native.lib().ldpc_bp_ensemble_decode_dev(n, dv, dc, check_lookup.data_ptr(), variable_lookup.data_ptr(),
                                                   llr.data_ptr(), B, max_iters, ALGOS[algo], float(alpha),
                                                   int(bool(early_stop)), _ptr(post), _ptr(hard), _ptr(its),
                                                   _stream(stream))
    _native.check(rc, "ldpc_bp_ensemble_decode_dev")
    return post, hard, its


# ------------------------------------------------------------- Gallager A/B
GALLAGER = "gallager"  # MonteCarlo(algo=GALLAGER): no ALGOS entry, the soft entry points never see it


def _flip_threshold(b):
    """The flip threshold of a Gallager A/B call: an integer 0 (Gallager A) .. 14."""
    if isinstance(b, bool) or int(b) != b or not 0 <= int(b) <= 14:
        raise ValueError(f"flip_threshold must be an integer 0 (Gallager A) .. 14, not {b!r}")
    return int(b)


def gallager_decode_dev(graph, bits, max_iters, flip_threshold=0, early_stop=False, hard=None, its=None, stream=None,
                        want_hard=True, want_its=True):
    """Gallager A (flip_threshold = 0) / B hard-decision decoding on the BSC, bit-exact with the
    definition in include/ldpc_mi355x.h.  bits: uint8 [B, n] device tensor of received words (bit
    0 of each byte is read).  Returns (hard uint8 [B, n], its int32 [B]) device tensors (None where
    not wanted)."""
    torch = _torch()
    B = bits.shape[0]
    assert bits.dtype == torch.uint8 and bits.is_contiguous() and bits.shape[1] == graph.n
    if hard is None and want_hard:
        hard = torch.empty_like(bits)
    if its is None and want_its:
        its = torch.empty((B,), dtype=torch.int32, device=bits.device)
    rc = _native.lib().ldpc_gb_decode_batch_dev(graph.handle(), bits.data_ptr(), B, int(max_iters),
                                                int(flip_threshold), int(bool(early_stop)), _ptr(hard), _ptr(its),
                                                _stream(stream))
    _native.check(rc, "ldpc_gb_decode_batch_dev")
    return hard, its


def gallager_decode(graph, bits, max_iters, flip_threshold=0, early_stop=False):
    """Host form: bits uint8 [B, n] numpy.  Returns (hard, its) numpy."""
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(bits), dtype=np.uint8)).cuda()
    hard, its = gallager_decode_dev(graph, t, max_iters, flip_threshold, early_stop)
    torch.cuda.synchronize()
    return hard.cpu().numpy(), its.cpu().numpy()


# ------------------------------------------------------------------ channels
def channel_dev(kind, param, seed, first_cw, n, B, out=None, stream=None, device=None, codewords=None,
                rate_match=None, known_llr=1024.0):
    """Channel outputs for codewords first_cw..first_cw+B-1: BEC -> uint8 (0 / 1 / 2 erasure),
    BSC / AWGN -> float32 LLRs.  codewords=None: the all-zero codeword (ldpc_channel_dev);
    codewords: uint8 [B, n] device tensor of transmitted 0/1 words -- the same stream reflected where
    the bit is 1 (ldpc_channel_cw_dev: the same erasures, LLRs exactly negated).
    rate_match: a ratematch.RateMatch (ldpc_channel_rm_dev) -- the transmitted positions as above, a
    punctured one an erasure / +0.0, a known one its bit / +-known_llr."""
    torch = _torch()
    kind = CHANNELS[kind]
    if out is None:
        dt = torch.uint8 if kind == CH_BEC else torch.float32
        out = torch.empty((B, n), dtype=dt, device=device or "cuda")
    if rate_match is not None:
        rm = rate_match
        if rm.n != n:
            raise ValueError(f"the rate-matching description is of n = {rm.n}, the channel of n = {n}")
        if codewords is not None:
            assert codewords.dtype == torch.uint8 and codewords.is_contiguous() and tuple(codewords.shape) == (B, n)
        rc = _native.lib().ldpc_channel_rm_dev(rm.handle(), kind, float(param), float(known_llr), int(seed),
                                               int(first_cw), B, _ptr(codewords), out.data_ptr(), _stream(stream))
        _native.check(rc, "ldpc_channel_rm_dev")
        return out
    if codewords is not None:
        assert codewords.dtype == torch.uint8 and codewords.is_contiguous() and tuple(codewords.shape) == (B, n)
        rc = _native.lib().ldpc_channel_cw_dev(kind, float(param), int(seed), int(first_cw), n, B,
                                               codewords.data_ptr(), out.data_ptr(), _stream(stream))
        _native.check(rc, "ldpc_channel_cw_dev")
        return out
    rc = _native.lib().ldpc_channel_dev(kind, float(param), int(seed), int(first_cw), n, B, out.data_ptr(),
                                        _stream(stream))
    _native.check(rc, "ldpc_channel_dev")
    return out
