"""Rate matching: which variables of a code are transmitted, punctured or known (shortened), and
which are counted (include/ldpc_mi355x.h, "Rate matching"; csrc/rate_match_host.cpp, csrc/rate_match.hip).

``RateMatch(n, punctured, shortened, count)`` describes a length-n code as its standard sends it: a
punctured variable is not transmitted and reaches the decoder as an erasure (BEC) or an LLR of +0
(BSC, BI-AWGN); a shortened variable is not transmitted either, its bit is a known 0, and it reaches
the decoder as that bit (BEC) or as +known_llr.  ``decoder.channel_dev(rate_match=)`` writes such
channel outputs, ``MonteCarlo(rate_match=)`` runs whole trials and counts the positions of the count
mask, ``QCCode.rate_match`` describes whole block columns.  The rate is (K - n_known) / n_tx.
"""
import ctypes as ct
import hashlib

import numpy as np

from . import _native
from ._native import RM_KNOWN, RM_PUNCT, RM_TX  # noqa: F401

COUNTS = ("codeword", "info")
KNOWN_LLR = 1024.0  # saturates every decoder of the library (the header's contract)


def pack(cls, count=None):
    """(packed uint8 [4 ceil(n / 4)], info int32 [5] = n, n_tx, n_punct, n_known, n_count) of
    ldpc_debug_rate_match_pack: validation and the device bytes, host only (no device)."""
    cls = np.ascontiguousarray(cls, np.uint8)
    n = cls.size
    cnt = None if count is None else np.ascontiguousarray(count, np.uint8)
    if cnt is not None and cnt.size != n:
        raise ValueError("rate matching: the count mask has another length than the classes")
    packed = np.zeros(4 * ((n + 3) // 4), np.uint8)
    info = np.zeros(5, np.int32)
    rc = _native.lib().ldpc_debug_rate_match_pack(n, cls.ctypes.data, None if cnt is None else cnt.ctypes.data,
                                                  packed.ctypes.data, info.ctypes.data)
    _native.check(rc, "ldpc_debug_rate_match_pack")
    return packed, info


def _positions(what, sel, n):
    """Sorted unique indices of an index list or a boolean mask of length n."""
    a = np.asarray(sel)
    if a.dtype == bool:
        if a.shape != (n,):
            raise ValueError(f"RateMatch: the {what} mask must have length n = {n}")
        return np.flatnonzero(a).astype(np.int64)
    if a.size == 0:
        return np.zeros(0, np.int64)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"RateMatch: {what} must be a list of indices or a boolean mask")
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= n:
        raise ValueError(f"RateMatch: a {what} index outside [0, {n})")
    u, c = np.unique(a, return_counts=True)
    if (c > 1).any():
        raise ValueError(f"RateMatch: {what} index {int(u[c > 1][0])} given twice")
    return u


class RateMatch:
    """punctured, shortened: index lists or boolean masks [n].  count: "codeword" (every position that
    is not known: the default of the C ABI), "info" (the information positions of the Encoder it is
    used with that are not known; resolved at use: MonteCarlo binds its graph's encoder, bind() does
    it by hand), or a 0/1 mask [n]."""

    def __init__(self, n, punctured=(), shortened=(), count="codeword"):
        if isinstance(n, bool) or int(n) != n or int(n) < 1:
            raise ValueError("RateMatch: need an integer n >= 1")
        self.n = int(n)
        p, s = _positions("punctured", punctured, self.n), _positions("shortened", shortened, self.n)
        both = np.intersect1d(p, s)
        if both.size:
            raise ValueError(f"RateMatch: index {int(both[0])} is both punctured and shortened")
        self.punctured, self.shortened = p, s
        self.cls = np.zeros(self.n, np.uint8)
        self.cls[p] = RM_PUNCT
        self.cls[s] = RM_KNOWN
        self.cls.setflags(write=False)
        if isinstance(count, str):
            if count not in COUNTS:
                raise ValueError(f"RateMatch: count must be one of {COUNTS} or a mask, not {count!r}")
            self.count, self._mask = count, None
        else:
            m = np.asarray(count)
            if m.shape != (self.n,) or not np.isin(m, (0, 1)).all():
                raise ValueError(f"RateMatch: a count mask must be [n = {self.n}] of 0 / 1")
            self.count, self._mask = "mask", m.astype(np.uint8)
        self._handles = {}  # (device, digest) -> ldpc_rate_match*
        self._encoder = None

    def bind(self, encoder):
        """The Encoder whose info_positions count="info" means, where none is passed.  Returns self."""
        if encoder.n != self.n:
            raise ValueError(f"RateMatch: the encoder's n = {encoder.n} is not the description's {self.n}")
        self._encoder = encoder
        return self

    n_punct = property(lambda self: int(self.punctured.size))
    n_known = property(lambda self: int(self.shortened.size))
    n_tx = property(lambda self: self.n - self.n_punct - self.n_known)

    def counts(self, encoder=None):
        """The count mask uint8 [n].  count="info" needs the Encoder whose information positions it means."""
        if self.count == "mask":
            return self._mask
        mask = (self.cls != RM_KNOWN).astype(np.uint8)
        if self.count == "info":
            encoder = encoder if encoder is not None else self._encoder
            if encoder is None:
                raise ValueError('RateMatch: count="info" is resolved against an Encoder (its info_positions)')
            if encoder.n != self.n:
                raise ValueError(f"RateMatch: the encoder's n = {encoder.n} is not the description's {self.n}")
            info = np.zeros(self.n, np.uint8)
            info[np.asarray(encoder.info_positions)] = 1
            mask &= info
        return mask

    def packed(self, encoder=None):
        return pack(self.cls, self.counts(encoder))[0]

    def digest(self, encoder=None):
        """SHA-1 of the packed device bytes: the description's identity in a snapshot."""
        return hashlib.sha1(self.packed(encoder).tobytes()).hexdigest()

    def rate(self, K):
        """(K - n_known) / n_tx, K the dimension of the mother code."""
        from . import de
        return de.rate_matched_rate(int(K), self.n_tx, self.n_known)

    def handle(self, encoder=None):
        """Device description (ldpc_rate_match*) on the current HIP device, created once per device."""
        from .decoder import _torch
        key = (_torch().cuda.current_device(), self.digest(encoder) if self.count == "info" else None)
        h = self._handles.get(key)
        if h is None:
            cls, cnt = np.ascontiguousarray(self.cls), np.ascontiguousarray(self.counts(encoder))
            h = ct.c_void_p()
            rc = _native.lib().ldpc_rate_match_create(self.n, cls.ctypes.data, cnt.ctypes.data, ct.byref(h))
            _native.check(rc, "ldpc_rate_match_create")
            self._handles[key] = h
        return h

    def info(self, encoder=None):
        """(n, n_tx, n_punct, n_known, n_count) as the device description reports them."""
        v = [ct.c_int32(0) for _ in range(5)]
        rc = _native.lib().ldpc_rate_match_info(self.handle(encoder), *[ct.addressof(x) for x in v])
        _native.check(rc, "ldpc_rate_match_info")
        return tuple(x.value for x in v)

    def __del__(self):
        try:
            if _native._lib is not None:
                for h in self._handles.values():
                    _native._lib.ldpc_rate_match_destroy(h)
        except Exception:
            pass
        self._handles = {}


def shortened_info_index(encoder, rm):
    """Indices j into the information bits with info_positions[j] shortened.  ValueError, naming the
    first offender, when a shortened position is a parity position of the encoder's elimination: its bit
    is a function of the information bits and cannot be set to 0."""
    if encoder.n != rm.n:
        raise ValueError(f"the encoder's n = {encoder.n} is not the description's {rm.n}")
    pos = np.asarray(encoder.info_positions, np.int64)
    is_info = np.zeros(rm.n, bool)
    is_info[pos] = True
    bad = rm.shortened[~is_info[rm.shortened]]
    if bad.size:
        raise ValueError(f"shortened position {int(bad[0])} is a parity position of the encoder, not an "
                         "information position: only information bits can be fixed to 0")
    return np.flatnonzero(rm.cls[pos] == RM_KNOWN)


def shorten_info(info, encoder, rm, index=None):
    """Zero, in place, the information bits [B, K] (numpy array or torch tensor) that sit at shortened
    positions, so that the encoded words are 0 there.  index: shortened_info_index(encoder, rm) where
    the caller keeps it (for a device tensor: on that device).  Returns info."""
    idx = shortened_info_index(encoder, rm) if index is None else index
    if len(idx) == 0:
        return info
    if isinstance(info, np.ndarray):
        info[:, np.asarray(idx)] = 0
        return info
    import torch
    return info.index_fill_(1, torch.as_tensor(idx, device=info.device), 0)
