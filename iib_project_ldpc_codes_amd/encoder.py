"""Systematic encoder of a fixed code on the MI355X (ldpc_encoder_*, csrc/encode_host.cpp and
csrc/encode.hip).

``Encoder(graph)`` eliminates H over GF(2) once on the host (rank, information and parity
positions, the dense parity matrix A) and uploads the tables; ``encode`` is P = A U bit-sliced over a
batch on the device.  ``random_codewords_dev`` draws the information bits of trials first_cw.. from
the library's Philox info stream (ldpc_info_bits_dev) and encodes them: the codewords that
MonteCarlo(codewords="random") transmits.
"""
import ctypes as ct

import numpy as np

from . import _native
from .decoder import _stream, _torch


def encode_rule():
    """Name of the elimination rule that fixes the positions and A (include/ldpc_mi355x.h)."""
    return _native.lib().ldpc_encode_rule().decode()


def host_description(check_ptr, check_var, n):
    """(rank, info_pos, par_pos, A_words uint32 [rank, ceil(K/32)]) of ldpc_debug_encoder_build: the
    elimination alone, host only (no device)."""
    cptr = np.ascontiguousarray(check_ptr, np.int32)
    cvar = np.ascontiguousarray(check_var, np.int32)
    m = cptr.size - 1
    rank = ct.c_int32(0)
    L = _native.lib()
    _native.check(L.ldpc_debug_encoder_build(cptr.ctypes.data, cvar.ctypes.data, n, m, ct.addressof(rank), None, None,
                                             None), "ldpc_debug_encoder_build")
    r, K = rank.value, n - rank.value
    info, par = np.zeros(K, np.int32), np.zeros(r, np.int32)
    A = np.zeros((r, (K + 31) // 32), np.uint32)
    _native.check(L.ldpc_debug_encoder_build(cptr.ctypes.data, cvar.ctypes.data, n, m, ct.addressof(rank),
                                             info.ctypes.data, par.ctypes.data, A.ctypes.data),
                  "ldpc_debug_encoder_build")
    return r, info, par, A


class Encoder:
    """Systematic encoder of a TannerGraph: x[info_positions] = u, x[parity_positions] = A u."""

    def __init__(self, graph):
        self.graph = graph
        self.n = graph.n
        self._handles = {}
        h = self.handle()
        n, K, r = ct.c_int32(0), ct.c_int32(0), ct.c_int32(0)
        _native.check(_native.lib().ldpc_encoder_info(h, ct.addressof(n), ct.addressof(K), ct.addressof(r)),
                      "ldpc_encoder_info")
        self.K, self.rank = K.value, r.value
        self.info_positions = np.zeros(self.K, np.int32)
        self.parity_positions = np.zeros(self.rank, np.int32)
        _native.check(_native.lib().ldpc_encoder_positions(h, self.info_positions.ctypes.data,
                                                           self.parity_positions.ctypes.data),
                      "ldpc_encoder_positions")

    def handle(self):
        """Device encoder (ldpc_encoder*) on the current HIP device, created once per device."""
        torch = _torch()
        dev = torch.cuda.current_device()
        h = self._handles.get(dev)
        if h is None:
            h = ct.c_void_p()
            _native.check(_native.lib().ldpc_encoder_create(self.graph.handle(), ct.byref(h)), "ldpc_encoder_create")
            self._handles[dev] = h
        return h

    def encode_dev(self, info, out=None, stream=None):
        """info: uint8 [B, K] device tensor (bit 0 of each byte is read).  Returns uint8 [B, n] of 0/1."""
        torch = _torch()
        assert info.dtype == torch.uint8 and info.is_contiguous() and info.dim() == 2 and info.shape[1] == self.K
        B = info.shape[0]
        if out is None:
            out = torch.empty((B, self.n), dtype=torch.uint8, device=info.device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (B, self.n)
        rc = _native.lib().ldpc_encode_batch_dev(self.handle(), info.data_ptr(), B, out.data_ptr(), _stream(stream))
        _native.check(rc, "ldpc_encode_batch_dev")
        return out

    def encode(self, info):
        """Host form: info uint8 [B, K] numpy.  Returns the codewords uint8 [B, n] numpy."""
        torch = _torch()
        u = np.ascontiguousarray(np.atleast_2d(info), dtype=np.uint8)
        out = self.encode_dev(torch.from_numpy(u).cuda())
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def info_bits_dev(self, seed, first_cw, B, out=None, stream=None):
        """The information bits uint8 [B, K] of trials first_cw .. first_cw + B - 1 (ldpc_info_bits_dev)."""
        torch = _torch()
        if out is None:
            out = torch.empty((B, self.K), dtype=torch.uint8, device="cuda")
        rc = _native.lib().ldpc_info_bits_dev(int(seed), int(first_cw), self.K, int(B), out.data_ptr(),
                                              _stream(stream))
        _native.check(rc, "ldpc_info_bits_dev")
        return out

    def random_codewords_dev(self, seed, first_cw, B, stream=None):
        """(codewords uint8 [B, n], info uint8 [B, K]) of trials first_cw .. first_cw + B - 1."""
        info = self.info_bits_dev(seed, first_cw, B, stream=stream)
        return self.encode_dev(info, stream=stream), info

    def __del__(self):
        try:
            if _native._lib is not None:
                for h in self._handles.values():
                    _native._lib.ldpc_encoder_destroy(h)
        except Exception:
            pass
        self._handles = {}
