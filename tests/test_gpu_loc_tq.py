"""bp_loc_chain_kernel<5, 512, TQ=500>: the chained fixed-count sum-product decode with its width a compile-time
constant (csrc/bp_loc_chain.hpp: the check phase's row offsets are instruction immediates, n and the copies' strides fold).

The shape is n = 10,000 (Tq = 500), the only one the instantiation accepts: 3 frames at sigma = 0.85, with 1, 2 and 7
iterations.  post, hard and its of the specialised launch must be np.array_equal to those of the generic
instantiation, run by a child process under LDPC_NO_LOC_TQ=1 (the switch is read when a graph's layouts are built;
the child asserts its plan names no width, the parent that its plan names 500): once on 16-byte-aligned rows, once
with llr and post starting one element into larger tensors (the narrow row path), once with post = None.  The
arithmetic and its order are the same in both instantiations, so nothing but equality is accepted.
A launch whose plan names a width that is not the graph's is refused by the launcher (LDPC_EHIP) and writes nothing.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, TQ, B, SIGMA = 10000, 500, 3, 0.85
ITERS = [1, 2, 7]
CASES = ["aligned", "offset1", "nopost"]
SWITCHES = ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T", "LDPC_NO_LOC_CHAIN", "LDPC_NO_LOC_TQ", "LDPC_NO_WIDE_IO")
F_SENT, H_SENT, I_SENT = -12345.5, 0xA5, -77


@functools.lru_cache(maxsize=None)
def _csr(n):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    return tuple(np.ascontiguousarray(a, np.int32) for a in TannerGraph.random_regular(n, 3, 6, seed=1).to_csr())


@functools.lru_cache(maxsize=None)
def _llr(n=N):
    llr = np.array(oracle.channel(oracle.CH_AWGN, SIGMA, 11, 0, n, B), np.float32)
    llr.setflags(write=False)
    return llr


def _plan(n, entry):
    """ldpc_debug_bp_plan_width / _tq of the fixed-count sum-product call, under the current environment."""
    from iib_project_ldpc_codes_amd import _native
    csr = _csr(n)
    calls, out = np.array([[B, 7, 0, 0, 0, 1]], np.int32), np.full(1, -1, np.int64)
    rc = getattr(_native.lib(), entry)(*(a.ctypes.data for a in csr), n, csr[0].size - 1, 1, calls.ctypes.data, 256,
                                       out.ctypes.data)
    assert rc == 0, _native.last_error()
    return int(out[0])


@functools.lru_cache(maxsize=None)
def _graph(n=N):
    """A handle whose layouts are built under the environment of this process's start but for the test switches
    that this module does not set itself; the chained layout exists at both shapes (seed 1)."""
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    g = TannerGraph.random_regular(n, 3, 6, seed=1)
    g.handle()
    assert g.kernel_name() == "bp_loc_kernel" and _plan(n, "ldpc_debug_bp_plan_width") == n // 20
    return g


def _wide(llr, post, hard):
    from iib_project_ldpc_codes_amd import _native
    csr = _csr(N)
    calls = np.array([[B, 7, 0, 0, 0, llr.data_ptr(), post.data_ptr() if post is not None else 0, hard.data_ptr(), 0]],
                     np.int64)
    out, names = np.zeros((1, 11), np.int64), np.zeros((1, 64), np.uint8)
    rc = _native.lib().ldpc_debug_bp_plan_io(*(a.ctypes.data for a in csr), N, csr[0].size - 1, 1, calls.ctypes.data,
                                             256, out.ctypes.data, names.ctypes.data)
    assert rc == 0, _native.last_error()
    return int(out[0, 9])


def _rows(torch, dtype, sentinel, skew, fill=None):
    """B rows of N elements starting `skew` elements into a sentinel-filled tensor."""
    buf = torch.full((B * N + 16,), sentinel, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[skew:skew + B * N].view(B, N)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _decode(torch, case, iters):
    """(post or None, hard, its) of one decode of the frames, as numpy."""
    from iib_project_ldpc_codes_amd import decoder
    skew = 1 if case == "offset1" else 0
    _, llr = _rows(torch, torch.float32, F_SENT, skew, torch.from_numpy(_llr().copy()).cuda())
    pbuf, post = _rows(torch, torch.float32, F_SENT, skew)
    hbuf, hard = _rows(torch, torch.uint8, H_SENT, 0)
    its = torch.full((B,), I_SENT, dtype=torch.int32, device="cuda")
    if case == "nopost":
        post = None
    assert _wide(llr, post, hard) == int(case != "offset1")
    decoder.bp_decode_dev(_graph(), llr, iters, "spa", post=post, hard=hard, its=its, want_post=post is not None)
    torch.cuda.synchronize()
    # nothing outside the rows was written
    assert np.all(pbuf.cpu().numpy()[:skew] == F_SENT) and np.all(pbuf.cpu().numpy()[skew + B * N:] == F_SENT)
    assert np.all(hbuf.cpu().numpy()[B * N:] == H_SENT)
    if post is None:
        assert np.all(pbuf.cpu().numpy() == F_SENT)
    return None if post is None else post.cpu().numpy(), hard.cpu().numpy(), its.cpu().numpy()


def _all_decodes(torch):
    out = {}
    for case in CASES:
        for iters in ITERS:
            post, hard, its = _decode(torch, case, iters)
            if post is not None:
                out[f"{case}_{iters}_post"] = post
            out[f"{case}_{iters}_hard"], out[f"{case}_{iters}_its"] = hard, its
    return out


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


@pytest.fixture(scope="module")
def generic(tmp_path_factory):
    """Every case's outputs from the generic instantiation: one child process under LDPC_NO_LOC_TQ=1."""
    path = str(tmp_path_factory.mktemp("loc_tq") / "generic.npz")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES and k != "WORLD_SIZE"}
    env["LDPC_NO_LOC_TQ"] = "1"
    p = subprocess.run([sys.executable, "-m", "tests.test_gpu_loc_tq", path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def special(torch):
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        assert _plan(N, "ldpc_debug_bp_plan_tq") == TQ
        _graph()
        return _all_decodes(torch)
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})


@pytest.mark.parametrize("case", CASES)
def test_specialised_equals_generic(special, generic, case):
    assert sorted(special) == sorted(generic)
    for iters in ITERS:
        keys = [f"{case}_{iters}_{w}" for w in (("hard", "its") if case == "nopost" else ("post", "hard", "its"))]
        for k in keys:
            a, b = special[k], generic[k]
            assert a.dtype == b.dtype and a.shape == b.shape
            assert np.array_equal(a, b), f"{k}: {np.sum(a != b)} of {a.size} values differ"
        assert np.all(special[f"{case}_{iters}_its"] == iters)
        if case != "nopost":
            post, hard = special[f"{case}_{iters}_post"], special[f"{case}_{iters}_hard"]
            assert np.all(np.isfinite(post)) and np.array_equal(hard, (post < 0).astype(np.uint8))
            # the three row forms agree with one another as well
            assert np.array_equal(post, special[f"aligned_{iters}_post"])
        assert np.array_equal(special[f"{case}_{iters}_hard"], special[f"aligned_{iters}_hard"])


def test_outputs_follow_the_oracle(special):
    """Not vacuous: the compared decodes are decodes (tests/test_gpu_loc_chain.py's tolerance)."""
    for iters in ITERS:
        opost, _, _ = oracle.bp_decode_batch(list(_csr(N)), _llr(), iters, 0)
        np.testing.assert_allclose(special[f"aligned_{iters}_post"], opost, rtol=1e-4, atol=1e-4)


def _forced(torch, n, tq, iters=2):
    """ldpc_debug_bp_decode_tq on the graph of n variables: (rc, post, hard, its) with sentinel-filled outputs."""
    from iib_project_ldpc_codes_amd import _native
    g = _graph(n)
    llr = torch.from_numpy(_llr(n).copy()).cuda()
    post = torch.full((B, n), F_SENT, dtype=torch.float32, device="cuda")
    hard = torch.full((B, n), H_SENT, dtype=torch.uint8, device="cuda")
    its = torch.full((B,), I_SENT, dtype=torch.int32, device="cuda")
    rc = _native.lib().ldpc_debug_bp_decode_tq(g.handle(), tq, llr.data_ptr(), B, iters, post.data_ptr(),
                                               hard.data_ptr(), its.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, post.cpu().numpy(), hard.cpu().numpy(), its.cpu().numpy()


def test_mismatching_plan_is_refused(torch, special):
    from iib_project_ldpc_codes_amd import _native
    # the entry itself: the plan's own width reproduces the decode, width 0 runs the generic instantiation
    for tq in (TQ, 0):
        rc, post, hard, its = _forced(torch, N, tq)
        assert rc == 0, _native.last_error()
        assert np.array_equal(post, special["aligned_2_post"]) and np.array_equal(hard, special["aligned_2_hard"])
        assert np.all(its == 2)
    # a width that is not the graph's: the specialised kernel on a Tq = 510 graph, an unlisted width, and the
    # generic graph's own width, which has no instantiation
    for n, tq in ((10200, TQ), (N, 510), (N, 499), (10200, 510)):
        rc, post, hard, its = _forced(torch, n, tq)
        assert rc == _native.LDPC_EHIP, (n, tq, rc)
        assert np.all(post == F_SENT) and np.all(hard == H_SENT) and np.all(its == I_SENT), (n, tq)
    # and the graph still decodes
    rc, post, _, _ = _forced(torch, N, TQ)
    assert rc == 0 and np.array_equal(post, special["aligned_2_post"])


if __name__ == "__main__":  # the child: python -m tests.test_gpu_loc_tq OUT.npz under LDPC_NO_LOC_TQ=1
    import torch as torch_
    assert os.environ.get("LDPC_NO_LOC_TQ") == "1" and _plan(N, "ldpc_debug_bp_plan_tq") == 0
    np.savez(sys.argv[1], **_all_decodes(torch_))
