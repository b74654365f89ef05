"""The staging and the epilogue of bp_loc_kernel's and bp_loc_chain_kernel's fixed-count decodes (the table loads and the LLR
copy issued together, the wire value from the one exponential; the posterior gathers from the
loop's positions, each variable id read once, the clamped-exponential test as one ballot with
its substitution pass behind it, the batched output reads) change no bit of any output.

Fixed-count sum-product decodes of (3,6) codes of n = 4,100 (the smallest chained shape: a
part-filled wave and idle waves) and n = 10,000 (the bench shape), 37 frames, 1, 2, 3 and 50
iterations, on the chained layout and (LDPC_NO_LOC_CHAIN=1) on the plain one, against
 * the oracle, within tests/test_gpu_loc_chain.py's tolerances, and
 * tests/golden/loc_fixed_cost_parent.json: the SHA-256 of post, hard and its of the same decodes
   by the build before this epilogue (its "how" field says how it was written).
Frame 5 holds channel values of 95 nats, whose exponentials clamp: its waves take the
substitution pass, every other wave the pass without it."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "loc_fixed_cost_parent.json")
SPA_RTOL, SPA_ATOL = 1e-4, 1e-4
SIZES = [4100, 10000]
ITERS = [1, 2, 3, 50]
B = 37
BIG = (0, 1, 17, 511, 512, 2049, -2, -1)  # variables of frame 5 with |LLR| = 95 nats


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


def _graph(n, chain):
    """A fresh handle whose layouts are built with or without the chained one."""
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    saved = {k: os.environ.pop(k, None) for k in ("LDPC_NO_LOC_LAYOUT", "LDPC_LOC_T", "LDPC_NO_LOC_CHAIN")}
    try:
        if not chain:
            os.environ["LDPC_NO_LOC_CHAIN"] = "1"
        g = TannerGraph.random_regular(n, 3, 6, seed=21)
        g.handle()  # the layouts are built now, under this environment
    finally:
        os.environ.pop("LDPC_NO_LOC_CHAIN", None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    assert g.kernel_name() == "bp_loc_kernel"
    return g


@functools.lru_cache(maxsize=None)
def _llr(n):
    llr = np.array(oracle.channel(oracle.CH_AWGN, 0.82, 5, 0, n, B), np.float32)
    big = list(BIG)
    llr[5, big] = np.where(llr[5, big] < 0, -95.0, 95.0).astype(np.float32)
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def _oracle(n, iters):
    from iib_project_ldpc_codes_amd.graph import TannerGraph
    csr = [np.ascontiguousarray(a, np.int32) for a in TannerGraph.random_regular(n, 3, 6, seed=21).to_csr()]
    return tuple(oracle.bp_decode_batch(csr, _llr(n), iters, 0))


def _digest(post, hard, its):
    h = hashlib.sha256()
    for a, t in ((post, np.float32), (hard, np.uint8), (its, np.int32)):
        h.update(np.ascontiguousarray(a, t).tobytes())
    return h.hexdigest()


def _key(n, chain, iters):
    return f"{'chain' if chain else 'plain'}_n{n}_it{iters}"


@pytest.mark.parametrize("chain", [True, False], ids=["chain", "plain"])
@pytest.mark.parametrize("n", SIZES)
def test_fixed_count_outputs_vs_oracle_and_parent_bits(torch, n, chain):
    from iib_project_ldpc_codes_amd import decoder
    with open(GOLDEN) as f:
        golden = json.load(f)["sha256"]
    g = _graph(n, chain)
    big = np.abs(_llr(n)[5]) > 90
    assert big.sum() == len(BIG)
    for iters in ITERS:
        post, hard, its = decoder.bp_decode(g, _llr(n), iters, "spa")
        opost, ohard, _ = _oracle(n, iters)
        print(f"{_key(n, chain, iters)}: max |post - oracle| {np.abs(post - opost).max():.3g}, "
              f"at the large-LLR variables {np.abs(post[5, big] - opost[5, big]).max():.3g}, "
              f"frames with the oracle's decisions {np.all(hard == ohard, axis=1).mean():.3f}")
        assert np.all(its == iters)
        if iters <= 3:
            np.testing.assert_allclose(post, opost, rtol=SPA_RTOL, atol=SPA_ATOL)
            clear = np.abs(opost) > 2 * SPA_ATOL  # a posterior within the tolerance of zero may take either sign
            assert np.array_equal(hard[clear], ohard[clear])
        else:  # test_chain_spa_50_iterations' criterion
            same = np.all(hard == ohard, axis=1)
            assert same.mean() >= 0.99
            d = np.abs(post[same].astype(np.float64) - opost[same])
            assert np.mean(d <= 1e-3 + 1e-3 * np.abs(opost[same])) >= 0.999
        assert _digest(post, hard, its) == golden[_key(n, chain, iters)], _key(n, chain, iters)


if __name__ == "__main__":  # LDPC_LIB_PATH=<the parent build's library> python -m tests.test_gpu_loc_fixed_cost OUT.json
    import sys
    from iib_project_ldpc_codes_amd import decoder
    sha = {}
    for n_ in SIZES:
        for chain_ in (True, False):
            g_ = _graph(n_, chain_)
            for iters_ in ITERS:
                sha[_key(n_, chain_, iters_)] = _digest(*decoder.bp_decode(g_, _llr(n_), iters_, "spa"))
    with open(sys.argv[1], "w") as f:
        json.dump({"how": "python -m tests.test_gpu_loc_fixed_cost OUT.json on one MI355X with LDPC_LIB_PATH at the "
                          "library built from the commit before the fixed-count epilogue (7ac55d8): SHA-256 over "
                          "post (float32), hard (uint8), its (int32) of each decode",
                   "sha256": sha}, f, indent=1)
        f.write("\n")
