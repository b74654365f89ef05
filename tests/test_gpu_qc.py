"""Quasi-cyclic codes on the device: bp_qc_q_kernel (csrc/bp_qc_q.hip) against the numpy reference
of the fixed-point contract (tests/layered_q_ref.py) on layer = check // Z, and against
bp_layer_q_kernel on the same graph and schedule (LDPC_NO_QC_KERNEL=1 at creation); the fp32
layered kernel on the block-row schedule against tests/layered_ref.py.  Every fixed-point value is
an integer: post, hard and its are bit-exact or wrong.

The codes (tests/qc_util.py) are the smallest shapes at which the kernel can go wrong:
    arr36_z7                n = 42: 64 threads; nearly every index wraps
    rnd36_z64, rnd36_z65    the thread-count boundary
    arr36_z67               n = 402: 256 threads, one partial step
    arr36_z307              n = 1,842: two steps, the second a tail of 51
    hand_z31                masked 4 x 12 with shifts 0 and Z - 1, block-row degrees 1, 2, 5, 8 (the
                            degree-1 rule m2 = Q; mixed degrees across layers)
    dense2x12_z37           16 wide
    dense2x20_z23           32 wide, two-word records
    mix3x12_z67             n = 804: 256 threads and 16 wide, block rows of degree 12, 9 and 5 (absent
                            edges on a wide instantiation)
    rnd3x20_z257            n = 5,140: 256 threads and 32 wide; Z = 257 is two checks per thread
                            with a tail of one
    z1                      Z = 1: the base is H itself
Every case first holds the launch plan of its own calls to the kernel name it claims.
"""
import ctypes as ct
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import codeword_util as cu
from tests import layered_q_ref, layered_ref
from tests import stream_util as su
from tests.graph_util import extreme_llrs
from tests.qc_util import code, graph, kernel_name, qc_plans, table_kernels
from tests.test_gpu_layered_q import SETS

pytestmark = pytest.mark.gpu

B, ITERS = 24, 20
NAMES = ["arr36_z7", "rnd36_z64", "rnd36_z65", "arr36_z67", "arr36_z307", "hand_z31", "dense2x12_z37",
         "dense2x20_z23", "z1", "mix3x12_z67", "rnd3x20_z257"]
KERNEL = {"arr36_z7": "bp_qc_q_kernel<64,8>", "rnd36_z64": "bp_qc_q_kernel<64,8>", "rnd36_z65": "bp_qc_q_kernel<256,8>",
          "arr36_z67": "bp_qc_q_kernel<256,8>", "arr36_z307": "bp_qc_q_kernel<256,8>", "hand_z31": "bp_qc_q_kernel<64,8>",
          "dense2x12_z37": "bp_qc_q_kernel<64,16>", "dense2x20_z23": "bp_qc_q_kernel<64,32>",
          "z1": "bp_qc_q_kernel<64,8>", "mix3x12_z67": "bp_qc_q_kernel<256,16>",
          "rnd3x20_z257": "bp_qc_q_kernel<256,32>"}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    t.cuda.set_device(0)
    return t


def _quant(params):
    from iib_project_ldpc_codes_amd.decoder import Quant
    return Quant(*params)


@functools.lru_cache(maxsize=None)
def _table_graph(name):
    """The same code kept on the table kernels: bp_layer_q_kernel on the block-row schedule."""
    with table_kernels():
        g = code(name).graph()
        g.handle()
    return g


def _routed(name, calls):
    c = code(name)
    plans = qc_plans(c, calls)
    for call, p in zip(calls, plans):
        assert p["name"] == kernel_name(c) == KERNEL[name], (name, call, p)
        assert p["grid"] == call[5] and p["threads"] == (64 if c.Z <= 64 else 256), (name, call, p)
    with table_kernels():
        assert all(p["name"].startswith("bp_layer_q_kernel<") for p in qc_plans(c, calls))
    return plans


def _layer(name):
    return np.arange(code(name).m) // code(name).Z


@functools.lru_cache(maxsize=None)
def _awgn(n):
    return oracle.channel(oracle.CH_AWGN, 0.80, 13, 0, n, B)


def _decode(g, llr, iters, params, early_stop=False):
    from iib_project_ldpc_codes_amd import decoder
    return decoder.bp_decode(g, llr, iters, "minsum", 1.0, early_stop, schedule="layered", quant=_quant(params))


def _assert_bit_exact(got, want, what):
    post, hard, its = got
    assert post.dtype == np.int8 and hard.dtype == np.uint8 and its.dtype == np.int32
    np.testing.assert_array_equal(hard, want[1], err_msg=str(what))
    np.testing.assert_array_equal(its, want[2], err_msg=str(what))
    np.testing.assert_array_equal(post, want[0], err_msg=str(what))


# ------------------------------------------------------------------- decodes
@pytest.mark.parametrize("params", SETS)
@pytest.mark.parametrize("name", NAMES)
def test_bit_exact(torch, name, params):
    g = graph(name)
    _routed(name, [(1, es, 0, 1, ITERS, B) for es in (0, 1)])
    L = _native().ldpc_graph_layer_rule
    assert L(g.handle()).decode() == L(_table_graph(name).handle()).decode() == "qc/block-row/v1"
    llr = _awgn(g.n)
    for early_stop in (False, True):
        want = layered_q_ref.decode(g.csr, _layer(name), llr, ITERS, *params, early_stop=early_stop)
        got = _decode(g, llr, ITERS, params, early_stop)
        _assert_bit_exact(got, want, (name, params, early_stop))
        _assert_bit_exact(_decode(_table_graph(name), llr, ITERS, params, early_stop), got, (name, params, "table"))


def _native():
    from iib_project_ldpc_codes_amd import _native
    return _native.lib()


def _same_floats(got, want, what):
    """Bit-equal floats; NaN where the reference has NaN (a NaN's sign and payload are not compared)."""
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=str(what))
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg=str(what))


@pytest.mark.parametrize("name", ["arr36_z67", "hand_z31"])
def test_fp32_layered_on_the_block_rows(torch, name):
    """bp_layer_kernel on the block-row tables: min-sum bit-exact, sum-product within 1e-4 + 1e-4 |x|
    (tests/test_gpu_layered.py's SPA_ATOL / SPA_RTOL, unsaturated: asserted).  hand_z31's block row 0
    is one circulant: a degree-1 check sends +inf in fp32 (the exclusive minimum, or product, of no
    input), so the 31 variables of block column 11, which no other check holds, are inf after the
    first iteration and inf - inf = NaN from the second on, in the reference and on the device alike."""
    from iib_project_ldpc_codes_amd import decoder
    g, Z = graph(name), code(name).Z
    lone = np.zeros(g.n, bool)
    if name == "hand_z31":
        lone[11 * Z:12 * Z] = True
    llr = _awgn(g.n)
    with np.errstate(all="ignore"):
        for early_stop in (False, True):
            want = layered_ref.decode(g.csr, _layer(name), llr, ITERS, 1, 0.75, early_stop)
            np.testing.assert_array_equal(np.isnan(want[0]), np.broadcast_to(lone, want[0].shape))
            post, hard, its = decoder.bp_decode(g, llr, ITERS, "minsum", 0.75, early_stop, schedule="layered")
            _same_floats(post, want[0], (name, early_stop))
            np.testing.assert_array_equal(hard, want[1])
            np.testing.assert_array_equal(its, want[2])
        frames = oracle.channel(oracle.CH_AWGN, 1.1, 21, 0, g.n, 8)
        want = layered_ref.decode(g.csr, _layer(name), frames, 3, 0)
    np.testing.assert_array_equal(np.isnan(want[0]), np.broadcast_to(lone, want[0].shape))
    assert np.abs(want[0][:, ~lone]).max() < layered_ref.XMAX  # nothing at the clamp
    post, hard, its = decoder.bp_decode(g, frames, 3, "spa", schedule="layered")
    np.testing.assert_allclose(post, want[0], rtol=1e-4, atol=1e-4)  # NaN where the reference has NaN
    assert np.all(its == 3)


def test_boundary_calls(torch):
    """max_iters = 0 returns the quantised channel values with its = 0 (NaN, +-inf, -0 and denormals
    through the quantiser); post or hard may be None; B = 0 does nothing; B = 1."""
    from iib_project_ldpc_codes_amd import decoder
    name, params = "arr36_z67", (6, 8, 2.0, 6, 0)
    g, q = graph(name), _quant(params)
    llr = extreme_llrs(g.n, B, 11)
    llr[:, 1::97] = np.nan
    llr[:, 2::89] = np.float32(1e-40)
    llr[:, 4::79] = np.inf
    llr[:, 5::73] = -np.inf
    _routed(name, [(1, 1, 0, 1, 0, B), (1, 1, 0, 0, 3, B), (1, 0, 0, 1, 3, 1)])
    post, hard, its = _decode(g, llr, 0, params, True)
    c = layered_q_ref.quantise(llr, params[2], q.Q)
    np.testing.assert_array_equal(post, c)
    np.testing.assert_array_equal(hard, c < 0)
    assert np.all(its == 0) and post.dtype == np.int8

    def ref(frames, iters, es=False):
        return layered_q_ref.decode(g.csr, _layer(name), frames, iters, *params, early_stop=es)
    t = torch.from_numpy(llr).cuda()
    post, hard, its = decoder.bp_decode_dev(g, t, 3, "minsum", 1.0, True, want_post=False, schedule="layered", quant=q)
    torch.cuda.synchronize()
    want = ref(llr, 3, True)
    assert post is None
    np.testing.assert_array_equal(hard.cpu().numpy(), want[1])
    np.testing.assert_array_equal(its.cpu().numpy(), want[2])
    post, hard, its = decoder.bp_decode_dev(g, t, 3, "minsum", 1.0, False, want_hard=False, schedule="layered", quant=q)
    torch.cuda.synchronize()
    assert hard is None
    np.testing.assert_array_equal(post.cpu().numpy(), ref(llr, 3)[0])
    post, hard, its = decoder.bp_decode_dev(g, t[:0], 3, "minsum", schedule="layered", quant=q)
    torch.cuda.synchronize()
    assert post.shape == (0, g.n) and its.shape == (0,)
    _assert_bit_exact(_decode(g, llr[:1], 3, params), ref(llr[:1], 3), "B = 1")


def test_refusals(torch):
    from iib_project_ldpc_codes_amd import _native, qc
    L = _native.lib()
    out = ct.c_void_p()
    wide = np.zeros((2, 33), np.int32)  # a block row of 33 circulants
    assert L.ldpc_graph_create_qc(2, 33, 2, wide.ctypes.data, ct.byref(out)) == _native.LDPC_EINVAL
    assert out.value is None
    # a block past the LDS cap: the (3,6) array code of Z = 8,887 (tests/test_qc_plan.py: 8,867 is the last that fits)
    big = qc.array_code(3, 6, 8887).graph()
    good = _native.Quant(2.0, 6, 8, 6, 0)
    llr = torch.zeros((1, big.n), dtype=torch.float32, device="cuda")
    its = torch.zeros(1, dtype=torch.int32, device="cuda")
    counters = torch.zeros(4 + 6, dtype=torch.int64, device="cuda")
    assert L.ldpc_bp_layered_q_decode_batch_dev(big.handle(), llr.data_ptr(), 1, 3, ct.addressof(good), 0, None, None,
                                                its.data_ptr(), None) == _native.LDPC_EUNSUP
    assert L.ldpc_mc_layered_q_batch_dev(big.handle(), _native.CH_BSC, 0.05, 1, 0, 8, 5, ct.addressof(good), 1, -1, 0,
                                         counters.data_ptr(), None) == _native.LDPC_EUNSUP
    torch.cuda.synchronize()


# --------------------------------------------------------------- Monte-Carlo
# 512 trials, so that a stop at 200 frame errors falls inside the batch: the reference (on the CPU,
# before the assertions were written) counts 491 frame errors on arr36_z307, 309 on arr36_z7 and 415
# on mix3x12_z67 (the 256-thread, 16-wide kernel in the all-zero mode; the stop falls at trial 248)
MC_B, MC_ITERS = 512, 20
MC_CASES = [("arr36_z307", 0.05, (6, 8, 2.0, 6, 0)), ("arr36_z7", 0.08, (5, 7, 2.0, 8, 1)),
            ("mix3x12_z67", 0.02, (5, 7, 2.0, 8, 1))]


def _mc_counters(g, p, params, early_stop, expurgation=-1, stop=0):
    import torch
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    mc = MonteCarlo(g, "bsc", p, MC_ITERS, algo="minsum", early_stop=early_stop, seed=8, batch=MC_B,
                    expurgation=expurgation, schedule="layered", quant=_quant(params))
    mc.run_batch(0, MC_B, stop)
    torch.cuda.synchronize()
    return mc.counters.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mc_ref(name, p, params, early_stop):
    llr = oracle.channel(oracle.CH_BSC, p, 8, 0, code(name).n, MC_B)
    _, _, its, curve, _ = layered_q_ref.decode(graph(name).csr, _layer(name), llr, MC_ITERS, *params,
                                               early_stop=early_stop)
    return its, curve


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name,p,params", MC_CASES)
def test_mc_bsc_exact(torch, name, p, params, early_stop):
    _routed(name, [(1, int(early_stop), 1, 0, MC_ITERS, MC_B)])
    its, curve = _mc_ref(name, p, params, early_stop)
    want = layered_q_ref.mc_counters(curve, its)
    assert want[0] == MC_B and 0 < want[1] < MC_B  # both decoded and failed frames
    got = _mc_counters(graph(name), p, params, early_stop)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_mc_counters(_table_graph(name), p, params, early_stop), want)


@pytest.mark.parametrize("name,p,params", MC_CASES)
def test_mc_expurgation_and_stop_inside_the_batch(torch, name, p, params):
    """Expurgation at the smallest final error count that occurs, and a stop at 200 frame errors
    inside the batch (the reference alone says so)."""
    its, curve = _mc_ref(name, p, params, True)
    final = curve[:, -1]
    X, stop = int(final[final > 0].min()), 200
    want = layered_q_ref.mc_counters(curve, its, X, stop)
    assert want[1] == stop and want[0] < MC_B and np.any((final > 0) & (final <= X))
    got = _mc_counters(graph(name), p, params, True, expurgation=X, stop=stop)
    np.testing.assert_array_equal(got, want)


def test_mc_random_codewords(torch):
    """MonteCarlo(codewords="random") on a quasi-cyclic graph: the generic encoder, the reflected
    BSC stream and the fixed-point layered decode, against the host chain of tests/codeword_util.py."""
    from iib_project_ldpc_codes_amd import encoder
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    from tests import encode_ref
    name, p, batch = "arr36_z67", 0.05, 64
    g = graph(name)
    cptr, cvar = g.csr[0], g.csr[1]
    rank, info, par, _ = encoder.host_description(cptr, cvar, g.n)
    x = encode_ref.solve(encode_ref.parity_matrix(cptr, cvar, g.n), info, par, cu.info_bits(cu.SEED, 0, batch, info.size))
    assert x.any() and not (encode_ref.parity_matrix(cptr, cvar, g.n).astype(np.int64) @ x.T % 2).any()
    llr = oracle.channel(oracle.CH_BSC, p, cu.SEED, 0, g.n, batch)
    llr = np.where(x == 1, -llr, llr).astype(np.float32)
    hard, its = layered_q_ref.decode(g.csr, _layer(name), llr, cu.ITERS, *cu.QUANT, early_stop=True)[1:3]
    want = layered_q_ref.mc_counters(cu.curves(x, llr, hard), np.asarray(its, np.int64))
    assert 0 < want[1] < batch  # some frames fail, some do not
    _routed(name, [(1, 1, 0, 0, cu.ITERS, batch)])
    mc = MonteCarlo(g, "bsc", p, cu.ITERS, early_stop=True, seed=cu.SEED, batch=batch, codewords="random",
                    algo="minsum", schedule="layered", quant=_quant(cu.QUANT))
    mc.run_batch(0, batch, 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mc.counters.cpu().numpy(), want)


# ------------------------------------------------------------------- streams
def test_two_queued_calls_on_one_stream(torch):
    """A fixed-count and an early-stop decode queued behind one stall on a side stream, no host
    synchronisation in between (tests/test_gpu_streams.py's method): late inputs, sentinel-filled
    outputs, a warm-up of the same shapes first."""
    from iib_project_ldpc_codes_amd import decoder
    from tests import index64_util as u
    su.calibrate(torch)
    name, frames = "arr36_z307", 8
    g = graph(name)
    g.handle()
    _routed(name, [(1, es, 0, 1, ITERS, frames) for es in (0, 1)])
    q = _quant(u.QUANT)

    def jobs(seed, first, want):
        llr_h = u.channel_rows(oracle.CH_BSC, 0.06, seed, u.true_indices(first, frames), g.n)
        out = []
        for es in (False, True):
            j = su.Job(torch, "qc layered_q es=%d" % es)
            llr = j.late_input(llr_h)
            w = layered_q_ref.decode(g.csr, _layer(name), llr_h, ITERS, *u.QUANT, early_stop=es)[:3] if want else (None,) * 3
            post = j.output((frames, g.n), torch.int8, w[0], "post")
            hard = j.output((frames, g.n), torch.uint8, w[1], "hard")
            its = j.output((frames,), torch.int32, w[2], "its")
            j.call(lambda s, es=es, llr=llr, post=post, hard=hard, its=its: decoder.bp_decode_dev(
                g, llr, ITERS, "minsum", 1.0, es, post=post, hard=hard, its=its, stream=s, schedule="layered", quant=q))
            out.append(j)
        return out

    S = su.side_streams(torch)[0]
    su.run_jobs(torch, jobs(977, 50000, False), S, "current", stalled=False)  # the warm-up
    queued = jobs(20261020, 1000, True)
    assert not su.run_jobs(torch, queued, S, "current"), "a queued call blocked the host (or the stall is too short)"
    for j in queued:
        j.check()
