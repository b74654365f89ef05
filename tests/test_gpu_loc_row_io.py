"""The row I/O of bp_loc_kernel's and bp_loc_chain_kernel's fixed-count decodes: the llr, post and hard rows go through buffer
descriptors whose range check stands in for per-element guards, 16 bytes at a time when the plan
finds the rows aligned (wide_io) and 4 bytes / 1 byte at a time otherwise (or under
LDPC_NO_WIDE_IO=1).

(3,6) at n = 4,100 (the smallest chained shape: a part-filled wave and idle waves, and every
thread's last groups past the row's end), 7 frames, on the chained layout and (LDPC_NO_LOC_CHAIN=1)
on the plain one; sum-product at 1 and 3 iterations, min-sum at 3.  Frame 5 holds channel values
of 95 nats (tests/test_gpu_loc_fixed_cost.py's frame: its waves take the substitution pass).
For each: the wide path's post, hard and its equal the forced-narrow path's bit for bit; so do
the outputs through views that start one float (llr, post) and one byte (hard) into larger
tensors, which the plan must send down the narrow path; post=None and hard=None each leave the
other outputs as they were.  Every output sits inside sentinel-filled memory -- a guard row before
and after, guard elements around the views -- and every sentinel must survive the call: that is
what holds the range check."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

N, B = 4100, 7
BIG = (0, 1, 17, 511, 512, 2049, -2, -1)  # variables of frame 5 with |LLR| = 95 nats
CASES = [("spa", 1), ("spa", 3), ("minsum", 3)]
F_SENT, H_SENT, I_SENT = -12345.5, 0xA5, -77


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


@functools.lru_cache(maxsize=None)
def _graph(chain):
    """A fresh handle whose layouts are built with or without the chained one."""
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    saved = {k: os.environ.pop(k, None) for k in ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T", "LDPC_NO_LOC_CHAIN")}
    try:
        if not chain:
            os.environ["LDPC_NO_LOC_CHAIN"] = "1"
        g = TannerGraph.random_regular(N, 3, 6, seed=21)
        g.handle()  # the layouts are built now, under this environment
    finally:
        os.environ.pop("LDPC_NO_LOC_CHAIN", None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    assert g.kernel_name() == "bp_loc_kernel"
    return g


@functools.lru_cache(maxsize=None)
def _llr():
    llr = np.array(oracle.channel(oracle.CH_AWGN, 0.82, 5, 0, N, B), np.float32)
    big = list(BIG)
    llr[5, big] = np.where(llr[5, big] < 0, -95.0, 95.0).astype(np.float32)
    llr.setflags(write=False)
    return llr


def _plan(chain, algo, iters, llr, post, hard, narrow):
    """(kernel name, wide_io, message LDS words) of the call, from the host plan."""
    from iib_project_ldpc_codes_amd import _native
    from iib_project_ldpc_codes_amd.decoder import ALGOS
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    csr = [np.ascontiguousarray(a, np.int32) for a in TannerGraph.random_regular(N, 3, 6, seed=21).to_csr()]
    ptr = lambda t: 0 if t is None else t.data_ptr()
    calls = np.array([[B, iters, ALGOS[algo], 0, 0, ptr(llr), ptr(post), ptr(hard), int(narrow)]], np.int64)
    out, names = np.zeros((1, 11), np.int64), np.zeros((1, 64), np.uint8)
    saved = os.environ.pop("LDPC_NO_LOC_CHAIN", None)
    if not chain:
        os.environ["LDPC_NO_LOC_CHAIN"] = "1"
    try:
        rc = _native.lib().ldpc_debug_bp_plan_io(*(a.ctypes.data for a in csr), N, csr[0].size - 1, 1, calls.ctypes.data,
                                                 256, out.ctypes.data, names.ctypes.data)
    finally:
        os.environ.pop("LDPC_NO_LOC_CHAIN", None)
        if saved is not None:
            os.environ["LDPC_NO_LOC_CHAIN"] = saved
    assert rc == 0, _native.last_error()
    return names[0].tobytes().split(b"\0")[0].decode(), int(out[0, 9]), int(out[0, 10])


class _Guarded:
    """B rows of `width` elements inside a sentinel-filled tensor: a guard row before and after,
    and `skew` guard elements between the first guard row and the rows (the view then starts `skew`
    elements past an aligned address)."""

    def __init__(self, torch, dtype, sentinel, width, skew, fill=None):
        self.torch, self.sentinel = torch, sentinel
        self.buf = torch.full(((B + 2) * width + 16,), sentinel, dtype=dtype, device="cuda")
        self.lo, self.hi = width + skew, width + skew + B * width
        self.view = self.buf[self.lo:self.hi].view(B, width) if width > 1 else self.buf[self.lo:self.hi]
        assert self.view.is_contiguous() and self.buf.data_ptr() % 256 == 0
        if fill is not None:
            self.view.copy_(fill)

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:self.lo] == self.sentinel) and np.all(b[self.hi:] == self.sentinel))


def _decode(torch, chain, algo, iters, skew=0, narrow=False, want_post=True, want_hard=True, expect_wide=None):
    """One decode into guarded outputs; returns (post, hard, its) as numpy (None where not asked for)."""
    from iib_project_ldpc_codes_amd import decoder
    llr = _Guarded(torch, torch.float32, F_SENT, N, skew, torch.from_numpy(_llr().copy()).cuda())
    post = _Guarded(torch, torch.float32, F_SENT, N, skew) if want_post else None
    hard = _Guarded(torch, torch.uint8, H_SENT, N, skew) if want_hard else None
    its = _Guarded(torch, torch.int32, I_SENT, 1, 0)
    pv, hv = post.view if post else None, hard.view if hard else None
    name, wide, words = _plan(chain, algo, iters, llr.view, pv, hv, narrow)
    assert name == "bp_loc_kernel" and words >= N + 4
    if expect_wide is not None:
        assert wide == int(expect_wide), (skew, narrow, wide)
    saved = os.environ.pop("LDPC_NO_WIDE_IO", None)
    if narrow:
        os.environ["LDPC_NO_WIDE_IO"] = "1"
    try:
        decoder.bp_decode_dev(_graph(chain), llr.view, iters, algo, post=pv, hard=hv, its=its.view,
                              want_post=want_post, want_hard=want_hard)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("LDPC_NO_WIDE_IO", None)
        if saved is not None:
            os.environ["LDPC_NO_WIDE_IO"] = saved
    for name_, t in (("llr", llr), ("post", post), ("hard", hard), ("its", its)):
        assert t is None or t.intact(), f"{name_}: a sentinel was overwritten (skew {skew}, narrow {narrow})"
    assert np.array_equal(llr.view.cpu().numpy(), _llr())
    return (pv.cpu().numpy() if post else None, hv.cpu().numpy() if hard else None, its.view.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _narrow(torch, chain, algo, iters):
    """The forced-narrow decode on aligned rows: the reference of every comparison, made once."""
    out = _decode(torch, chain, algo, iters, narrow=True, expect_wide=False)
    for a in out:
        a.setflags(write=False)
    return out


def _same(got, ref):
    return all(g is None or np.array_equal(g, r) for g, r in zip(got, ref))


@pytest.mark.parametrize("chain", [True, False], ids=["chain", "plain"])
@pytest.mark.parametrize("algo,iters", CASES)
def test_wide_path_equals_narrow(torch, chain, algo, iters):
    ref = _narrow(torch, chain, algo, iters)
    assert np.all(ref[2] == iters) and np.all(np.isfinite(ref[0])) and np.all(ref[1] <= 1)
    assert np.array_equal(ref[1], (ref[0] < 0).astype(np.uint8))
    assert _same(_decode(torch, chain, algo, iters, expect_wide=True), ref)


@pytest.mark.parametrize("chain", [True, False], ids=["chain", "plain"])
@pytest.mark.parametrize("algo,iters", CASES)
def test_unaligned_views_take_the_narrow_path(torch, chain, algo, iters):
    assert _same(_decode(torch, chain, algo, iters, skew=1, expect_wide=False), _narrow(torch, chain, algo, iters))


@pytest.mark.parametrize("chain", [True, False], ids=["chain", "plain"])
@pytest.mark.parametrize("algo,iters", CASES)
def test_null_outputs(torch, chain, algo, iters):
    ref = _narrow(torch, chain, algo, iters)
    for skew, wide in ((0, True), (1, False)):
        assert _same(_decode(torch, chain, algo, iters, skew=skew, want_post=False, expect_wide=wide), ref)
        assert _same(_decode(torch, chain, algo, iters, skew=skew, want_hard=False, expect_wide=wide), ref)
