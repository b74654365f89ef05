"""bp_loc_chain_kernel launched Tq threads wide (csrc/bp_loc_chain.hpp: no lane of it tests
tid < Tq, a part-filled last wave is the hardware's EXEC mask, and the LLR copy, the read-back and
the stores of post / hard stride by the launch width and cover each row exactly).

Fixed-count sum-product decodes of (3,6) codes, 37 frames, 1, 2, 3 and 50 iterations, at shapes
chosen by the last wave's fill:
  n =  5,120: Tq = 256, whole waves only;
  n =  5,140: Tq = 257, one live lane in the last wave;
  n = 10,200: Tq = 510, the largest that fits.
Each graph's chained layout is asserted to exist (ldpc_debug_loc_chain_layout, host only) before
anything is launched, and its launch width to be Tq.  Frame 5 holds channel values of 95 nats,
whose exponentials clamp, at variables of the first thread and of the last thread (Tq - 1, in the
part-filled wave where there is one): the substitution pass's ballot runs there.

Every case runs on aligned rows (16 bytes a load and a store) and on views that start 4 bytes into
larger tensors (the narrow path), with sentinels before and after every llr, post and hard row
range and around its; every sentinel must survive.  Outputs are checked
 * against the oracle, at tests/test_gpu_loc_chain.py's tolerances and its 50-iteration criterion, and
 * bit for bit against tests/golden/loc_chain_width_parent.json: the SHA-256 of post, hard and its
   of the same decodes by the build before this launch width (its "how" field says how it was written).
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "loc_chain_width_parent.json")
SPA_RTOL, SPA_ATOL = 1e-4, 1e-4
SHAPES = {5120: 256, 5140: 257, 10200: 510}  # n: Tq
SEED = 3  # chosen on the CPU: the path search of build_loc_chain_layout succeeds on these three graphs
ITERS = [1, 2, 3, 50]
B = 37
T, KP = 512, 5
F_SENT, H_SENT, I_SENT = -12345.5, 0xA5, -77
SKEW_BYTES = 4


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


@functools.lru_cache(maxsize=None)
def _csr(n):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    return tuple(np.ascontiguousarray(a, np.int32) for a in TannerGraph.random_regular(n, 3, 6, seed=SEED).to_csr())


@functools.lru_cache(maxsize=None)
def _layout(n):
    """(Tq, the variables of thread 0, the variables of thread Tq - 1) of the graph's chained layout; asserts it exists."""
    from iib_project_ldpc_codes_amd import _native
    csr = _csr(n)
    shape = np.zeros(6, np.int32)
    var = np.zeros(2 * KP * 2 * T, np.int32)
    rc = _native.lib().ldpc_debug_loc_chain_layout(*(a.ctypes.data for a in csr), n, csr[0].size - 1, shape.ctypes.data,
                                                   var.ctypes.data, None, None, None)
    assert rc == 0, f"n = {n}, seed {SEED}: no chained layout ({_native.last_error()})"
    Tq = int(shape[0])
    assert Tq == SHAPES[n] == n // 20 and int(shape[5]) == T
    var = var.reshape(2 * KP, 2, T)
    assert (var[:, :, :Tq] >= 0).all() and (var[:, :, Tq:] == -1).all()
    return Tq, var[:, :, 0].ravel().copy(), var[:, :, Tq - 1].ravel().copy()


def _big(n):
    """Variables of frame 5 with |LLR| = 95 nats: three of thread 0, three of the last thread."""
    _, first, last = _layout(n)
    return sorted({int(first[0]), int(first[7]), int(first[19]), int(last[0]), int(last[11]), int(last[19])})


@functools.lru_cache(maxsize=None)
def _llr(n):
    llr = np.array(oracle.channel(oracle.CH_AWGN, 0.82, 5, 0, n, B), np.float32)
    big = _big(n)
    llr[5, big] = np.where(llr[5, big] < 0, -95.0, 95.0).astype(np.float32)
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def _oracle(n, iters):
    return tuple(oracle.bp_decode_batch(list(_csr(n)), _llr(n), iters, 0))


@functools.lru_cache(maxsize=None)
def _graph(n):
    """A fresh handle with the chained layout, whose fixed-count sum-product plan launches Tq threads."""
    from iib_project_ldpc_codes_amd import _native
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    _layout(n)  # the layout exists: checked on the host before any launch
    saved = {k: os.environ.pop(k, None) for k in ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T", "LDPC_NO_LOC_CHAIN")}
    try:
        g = TannerGraph.random_regular(n, 3, 6, seed=SEED)
        g.handle()  # the layouts are built now, under this environment
        if hasattr(_native.lib(), "ldpc_debug_bp_plan_width"):  # not in the build that wrote the golden file
            csr = _csr(n)
            calls, out = np.array([[B, 50, 0, 0, 0, 1]], np.int32), np.zeros(1, np.int64)
            rc = _native.lib().ldpc_debug_bp_plan_width(*(a.ctypes.data for a in csr), n, csr[0].size - 1, 1,
                                                        calls.ctypes.data, 256, out.ctypes.data)
            assert rc == 0 and int(out[0]) == SHAPES[n]
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    assert g.kernel_name() == "bp_loc_kernel"
    return g


def _wide(n, iters, llr, post, hard):
    """wide_io of the call, from the host plan (ldpc_debug_bp_plan_io)."""
    from iib_project_ldpc_codes_amd import _native
    csr = _csr(n)
    calls = np.array([[B, iters, 0, 0, 0, llr.data_ptr(), post.data_ptr(), hard.data_ptr(), 0]], np.int64)
    out, names = np.zeros((1, 11), np.int64), np.zeros((1, 64), np.uint8)
    rc = _native.lib().ldpc_debug_bp_plan_io(*(a.ctypes.data for a in csr), n, csr[0].size - 1, 1, calls.ctypes.data,
                                             256, out.ctypes.data, names.ctypes.data)
    assert rc == 0, _native.last_error()
    assert names[0].tobytes().split(b"\0")[0].decode() == "bp_loc_kernel" and int(out[0, 1]) == T
    return int(out[0, 9])


class _Guarded:
    """B rows of `width` elements inside a sentinel-filled tensor: a guard row before and after, and
    `skew` guard elements between the first guard row and the rows."""

    def __init__(self, torch, dtype, sentinel, width, skew, fill=None):
        self.sentinel = sentinel
        self.buf = torch.full(((B + 2) * width + 16,), sentinel, dtype=dtype, device="cuda")
        self.lo, self.hi = width + skew, width + skew + B * width
        self.view = self.buf[self.lo:self.hi].view(B, width) if width > 1 else self.buf[self.lo:self.hi]
        assert self.view.is_contiguous() and self.buf.data_ptr() % 256 == 0
        if fill is not None:
            self.view.copy_(fill)

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:self.lo] == self.sentinel) and np.all(b[self.hi:] == self.sentinel))


def _decode(torch, n, iters, skewed):
    """One decode into guarded outputs, on aligned rows or on views SKEW_BYTES into their tensors."""
    from iib_project_ldpc_codes_amd import decoder
    sf, sh = (SKEW_BYTES // 4, SKEW_BYTES) if skewed else (0, 0)
    assert n % 4 == 0  # rows of n floats / n bytes keep the first row's alignment mod 16 / 4 bytes
    llr = _Guarded(torch, torch.float32, F_SENT, n, sf, torch.from_numpy(_llr(n).copy()).cuda())
    post = _Guarded(torch, torch.float32, F_SENT, n, sf)
    hard = _Guarded(torch, torch.uint8, H_SENT, n, sh)
    its = _Guarded(torch, torch.int32, I_SENT, 1, 0)
    assert _wide(n, iters, llr.view, post.view, hard.view) == int(not skewed)
    decoder.bp_decode_dev(_graph(n), llr.view, iters, "spa", post=post.view, hard=hard.view, its=its.view)
    torch.cuda.synchronize()
    for name, t in (("llr", llr), ("post", post), ("hard", hard), ("its", its)):
        assert t.intact(), f"{name}: a sentinel was overwritten (n {n}, {iters} iterations, skewed {skewed})"
    assert np.array_equal(llr.view.cpu().numpy(), _llr(n))
    return post.view.cpu().numpy(), hard.view.cpu().numpy(), its.view.cpu().numpy()


def _digest(post, hard, its):
    h = hashlib.sha256()
    for a, t in ((post, np.float32), (hard, np.uint8), (its, np.int32)):
        h.update(np.ascontiguousarray(a, t).tobytes())
    return h.hexdigest()


def _key(n, iters):
    return f"chain_n{n}_it{iters}"


@pytest.mark.parametrize("skewed", [False, True], ids=["aligned", "offset4"])
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_tq_wide_launch_vs_oracle_and_parent_bits(torch, n, skewed):
    with open(GOLDEN) as f:
        golden = json.load(f)["sha256"]
    big = np.abs(_llr(n)[5]) > 90
    assert big.sum() == len(_big(n)) == 6
    for iters in ITERS:
        post, hard, its = _decode(torch, n, iters, skewed)
        opost, ohard, _ = _oracle(n, iters)
        print(f"{_key(n, iters)} skewed {skewed}: max |post - oracle| {np.abs(post - opost).max():.3g}, "
              f"at the large-LLR variables {np.abs(post[5, big] - opost[5, big]).max():.3g}, "
              f"frames with the oracle's decisions {np.all(hard == ohard, axis=1).mean():.3f}")
        assert np.all(its == iters)
        assert np.all(np.isfinite(post)) and np.array_equal(hard, (post < 0).astype(np.uint8))
        if iters <= 3:
            np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL)
            clear = np.abs(opost) > 2 * SPA_ATOL  # a posterior within the tolerance of zero may take either sign
            assert np.array_equal(hard[clear], ohard[clear])
        else:  # test_chain_spa_50_iterations' criterion
            same = np.all(hard == ohard, axis=1)
            assert same.mean() >= 0.99
            d = np.abs(post[same].astype(np.float64) - opost[same])
            assert np.mean(d <= 1e-3 + 1e-3 * np.abs(opost[same])) >= 0.999
        assert _digest(post, hard, its) == golden[_key(n, iters)], _key(n, iters)


if __name__ == "__main__":  # in a checkout of the parent commit, with its library: python -m tests.test_gpu_loc_chain_width OUT.json
    import sys
    import torch as torch_
    sha = {}
    for n_ in sorted(SHAPES):
        for iters_ in ITERS:
            a_, s_ = _decode(torch_, n_, iters_, False), _decode(torch_, n_, iters_, True)
            assert all(np.array_equal(x, y) for x, y in zip(a_, s_)), (n_, iters_)
            sha[_key(n_, iters_)] = _digest(*a_)
    with open(sys.argv[1], "w") as f:
        json.dump({"how": "python -m tests.test_gpu_loc_chain_width OUT.json on one MI355X in a checkout of the parent "
                          "commit (e24ea5b: bp_loc_kernel's chained instantiation launched 512 threads wide) with "
                          "LDPC_LIB_PATH at the library built from it: SHA-256 over post (float32), hard (uint8), "
                          "its (int32) of each decode; the aligned and the 4-byte-offset decode agreed bit for bit",
                   "sha256": sha}, f, indent=1)
        f.write("\n")
