"""The codeword family on the device (csrc/encode.hip), every comparison bit-exact: the encoder
against tests/encode_ref.py's independent elimination, the information stream against the oracle's
Philox, the codeword channel against ldpc_channel_dev reflected, the counts against host arithmetic,
and the four entries in stream order behind a stall (tests/stream_util.py).
"""
import ctypes as ct

import numpy as np
import pytest

from oracle import oracle
from tests import encode_ref, encode_util as eu, gallager_ref
from tests.index64_util import SEED, T

pytestmark = pytest.mark.gpu

BATCHES = (1, 31, 32, 33, 257)  # a partial plane word, a whole one, a partial tile, more than one tile
M32 = T - 1


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch


def _info_bits(seed, first, B, K):
    """The header's information stream from the oracle's Philox, block by block."""
    out = np.zeros((B, K), np.uint8)
    key = [seed & M32, seed >> 32]
    for b in range(B):
        t = first + b
        for blk in range((K + 127) // 128):
            w = oracle.philox([blk, 1, t & M32, t >> 32], key)
            bits = (w[:, None] >> np.arange(32, dtype=np.uint32)[None, :] & 1).astype(np.uint8).ravel()
            j0 = 128 * blk
            out[b, j0:min(K, j0 + 128)] = bits[:min(K, j0 + 128) - j0]
    return out


# ------------------------------------------------------------------------------ 1. encode
@pytest.mark.parametrize("name", eu.GPU_NAMES)
def test_encode_against_reference(torch, name):
    from iib_project_ldpc_codes_amd.encoder import Encoder
    H = eu.H(name)
    n = H.shape[1]
    enc = Encoder(eu.tanner(name))
    rank, info, par, _ = eu.description(name)
    assert (enc.rank, enc.K) == (rank, n - rank)
    np.testing.assert_array_equal(enc.info_positions, info)
    np.testing.assert_array_equal(enc.parity_positions, par)
    U = np.random.default_rng(3).integers(0, 2, (max(BATCHES), enc.K)).astype(np.uint8)
    want = encode_ref.solve(H, info, par, U)  # once, for the largest batch: row b depends on U[b] alone
    for B in BATCHES:
        # bytes above bit 0 are not read
        u = U[:B] | (np.random.default_rng(B).integers(0, 128, (B, enc.K)).astype(np.uint8) << 1)
        x = enc.encode(u)
        assert x.shape == (B, n) and x.dtype == np.uint8
        np.testing.assert_array_equal(x, want[:B], err_msg="%s B=%d" % (name, B))
        np.testing.assert_array_equal(x[:, info], U[:B])
        assert not (H.astype(np.int64) @ x.T.astype(np.int64) & 1).any()  # H x = 0, every row
    if enc.K == 0:
        assert not enc.encode(np.zeros((33, 0), np.uint8)).any()


@pytest.mark.parametrize("name,W", eu.TILE_NAMES)
def test_encode_narrower_tiles(torch, name, W):
    """encode_parity_kernel<2> and <1> (every graph above runs <4>) at the smallest K that selects each,
    33 codewords (a whole plane word and one more): the plan first, then the reference bit for bit."""
    from iib_project_ldpc_codes_amd.encoder import Encoder
    H = eu.H(name)
    n = H.shape[1]
    enc = Encoder(eu.tanner(name))
    rank, info, par, _ = eu.description(name)
    assert (enc.rank, enc.K) == (rank, n - rank) == (16, n - 16)
    rc, rows = eu.encode_plans([(n, enc.K, rank, 33), (n - 1, enc.K - 1, rank, 33)])
    assert rc == 0 and [r["name"] for r in rows] == ["encode_parity_kernel<%d>" % W, "encode_parity_kernel<%d>" % (2 * W)]
    U = np.random.default_rng(3).integers(0, 2, (33, enc.K)).astype(np.uint8)
    want = encode_ref.solve(H, info, par, U)
    x = enc.encode(U)
    np.testing.assert_array_equal(x, want)
    assert not (H.astype(np.int64) @ x.T.astype(np.int64) & 1).any()


def test_encode_unaligned_output(torch):
    """An output that starts at an odd byte: the byte-store form (as for `lonely`, n = 97)."""
    from iib_project_ldpc_codes_amd.encoder import Encoder
    enc = Encoder(eu.tanner("r36_96"))
    rank, info, par, _ = eu.description("r36_96")
    U = np.random.default_rng(4).integers(0, 2, (33, enc.K)).astype(np.uint8)
    want = encode_ref.solve(eu.H("r36_96"), info, par, U)
    buf = torch.full((33 * 96 + 1,), 0x7F, dtype=torch.uint8, device="cuda")
    out = buf[1:].view(33, 96)
    enc.encode_dev(torch.from_numpy(U).cuda(), out=out)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert int(buf[0]) == 0x7F


# ------------------------------------------------------------------------- 2. info stream
@pytest.mark.parametrize("K", [1, 127, 129, 500])
def test_info_stream_against_philox(torch, K):
    from iib_project_ldpc_codes_amd import _native
    first, B = T - 3, 8  # trials straddling 2^32 under a seed above 2^32
    out = torch.full((B, K), 0x7F, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _native.check(_native.lib().ldpc_info_bits_dev(SEED, first, K, B, out.data_ptr(), s), "ldpc_info_bits_dev")
    got = out.cpu().numpy()
    want = _info_bits(SEED, first, B, K)
    np.testing.assert_array_equal(got, want)
    assert K == 1 or 0 < want.sum() < want.size
    # one trial drawn in two different batches is the same trial
    again = torch.full((3, K), 0x7F, dtype=torch.uint8, device="cuda")
    _native.check(_native.lib().ldpc_info_bits_dev(SEED, first + 4, K, 3, again.data_ptr(), s), "ldpc_info_bits_dev")
    np.testing.assert_array_equal(again.cpu().numpy(), got[4:7])
    # the seed's high word is part of the key
    if K == 500:
        other = _info_bits(SEED & M32, first, 1, K)
        assert (other != want[:1]).any()


# --------------------------------------------------------------------- 3. codeword channel
@pytest.mark.parametrize("n", [10, 1000])
@pytest.mark.parametrize("kind,param", [("bec", 0.4), ("bsc", 0.07), ("awgn", 0.8)])
@pytest.mark.parametrize("first", [5, T - 3])
def test_codeword_channel_is_the_reflection(torch, kind, param, n, first):
    from iib_project_ldpc_codes_amd import _native, decoder
    B = 8
    zero = decoder.channel_dev(kind, param, SEED, first, n, B)
    # d_cw = NULL: ldpc_channel_dev's output bit for bit
    same = torch.full_like(zero, 0x7F if kind == "bec" else 7.0)
    rc = _native.lib().ldpc_channel_cw_dev(decoder.CHANNELS[kind], param, SEED, first, n, B, None, same.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "ldpc_channel_cw_dev")
    x = np.random.default_rng(n).integers(0, 2, (B, n)).astype(np.uint8)
    refl = decoder.channel_dev(kind, param, SEED, first, n, B, codewords=torch.from_numpy(x).cuda())
    z, s, r = zero.cpu().numpy(), same.cpu().numpy(), refl.cpu().numpy()
    if kind == "bec":
        np.testing.assert_array_equal(s, z)
        np.testing.assert_array_equal(r, np.where(z == 2, 2, x))
        assert (z == 2).any() and (z == 0).any()
    else:
        np.testing.assert_array_equal(s.view(np.int32), z.view(np.int32))
        np.testing.assert_array_equal(r.view(np.int32), np.where(x == 1, -z, z).view(np.int32))  # an exact negation
        assert (z < 0).any() and (z > 0).any()
    if kind != "awgn":  # the oracle restates these two streams bit for bit (its BI-AWGN values differ in the last place)
        np.testing.assert_array_equal(z, oracle.channel(decoder.CHANNELS[kind], param, SEED, first, n, B).astype(z.dtype))


# ------------------------------------------------------------------------------ 4. counts
def _count_case(n, B, iters, seed):
    rs = np.random.default_rng(seed)
    cw = rs.integers(0, 2, (B, n)).astype(np.uint8)
    llr = rs.standard_normal((B, n)).astype(np.float32)
    llr[0, :3] = [0.0, -0.0, 1e-30]  # zero and minus zero are not negative
    hard = cw.copy()
    wrong = rs.integers(0, 7, B)  # final errors per trial, 0 .. 6: some frames correct, some at or below X = 3
    for b in range(B):
        hard[b, rs.permutation(n)[:wrong[b]]] ^= 1
    its = rs.integers(1, iters + 1, B).astype(np.int32)
    curve = np.zeros((B, iters + 1), np.int64)
    curve[:, 0] = ((llr < 0).astype(np.uint8) != cw).sum(axis=1)
    curve[:, iters] = (hard != cw).sum(axis=1)
    return cw, llr, hard, its, curve


@pytest.mark.parametrize("X", [-1, 3])
@pytest.mark.parametrize("llr_form", [True, False])
def test_counts_against_host_arithmetic(torch, X, llr_form):
    from iib_project_ldpc_codes_amd import _native
    n, B, iters = 203, 300, 6
    cw, llr, hard, its, curve = _count_case(n, B, iters, 11)
    frames = (curve[:, -1] > X) & (curve[:, -1] != 0)
    stop = int(frames[:B // 2].sum())  # reached in the middle of the batch
    assert 0 < stop < frames.sum()
    chan = llr if llr_form else (llr < 0).astype(np.uint8) | 0x40  # bits: bit 0 is read
    d = [torch.from_numpy(a).cuda() for a in (cw, chan, hard, its)]
    s = torch.cuda.current_stream().cuda_stream
    for st in (0, stop):
        base = np.arange(4 + iters + 1, dtype=np.int64) * 1000  # accumulated, interior entries not touched
        base[1] = 0  # the stop rule counts the frame errors already there
        counters = torch.from_numpy(base.copy()).cuda()
        rc = _native.lib().ldpc_mc_cw_count_dev(d[0].data_ptr(), d[1].data_ptr(), int(llr_form), d[2].data_ptr(),
                                                d[3].data_ptr(), n, B, iters, X, st, counters.data_ptr(), s)
        _native.check(rc, "ldpc_mc_cw_count_dev")
        want = gallager_ref.mc_counters(curve, its, X, st)
        np.testing.assert_array_equal(counters.cpu().numpy(), base + want)
        assert not want[5:4 + iters].any() and (st == 0 or want[0] < B)
    # max_iters = 0: the one curve entry takes the final errors; no iteration counts
    counters = torch.zeros(5, dtype=torch.int64, device="cuda")
    rc = _native.lib().ldpc_mc_cw_count_dev(d[0].data_ptr(), d[1].data_ptr(), int(llr_form), d[2].data_ptr(), None, n,
                                            B, 0, -1, 0, counters.data_ptr(), s)
    _native.check(rc, "ldpc_mc_cw_count_dev")
    f = curve[:, -1]
    assert counters.cpu().numpy().tolist() == [B, int((f != 0).sum()), int(f.sum()), 0, int(f.sum())]


# ---------------------------------------------------------------------- errors and no-ops
def test_error_returns_and_empty_batches(torch):
    from iib_project_ldpc_codes_amd import _native
    from iib_project_ldpc_codes_amd.encoder import Encoder
    L = _native.lib()
    enc = Encoder(eu.tanner("r36_96"))
    h, s = enc.handle(), torch.cuda.current_stream().cuda_stream
    buf = torch.full((4096,), 0x7F, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(9, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    EINVAL = _native.LDPC_EINVAL
    assert L.ldpc_encoder_create(None, ct.byref(ct.c_void_p())) == EINVAL
    assert L.ldpc_encoder_info(None, None, None, None) == EINVAL
    assert L.ldpc_encoder_positions(None, None, None) == EINVAL
    assert L.ldpc_encode_batch_dev(None, p, 1, p, s) == EINVAL
    assert L.ldpc_encode_batch_dev(h, p, -1, p, s) == EINVAL
    assert L.ldpc_encode_batch_dev(h, None, 1, p, s) == EINVAL
    assert L.ldpc_encode_batch_dev(h, p, 1, None, s) == EINVAL
    assert L.ldpc_info_bits_dev(1, 0, -1, 1, p, s) == EINVAL
    assert L.ldpc_info_bits_dev(1, 0, 8, -1, p, s) == EINVAL
    assert L.ldpc_info_bits_dev(1, 0, 8, 1, None, s) == EINVAL
    assert L.ldpc_channel_cw_dev(1, 0.6, 1, 0, 8, 1, None, p, s) == EINVAL  # the BSC's p must be below 0.5
    assert L.ldpc_channel_cw_dev(1, 0.1, 1, 0, 0, 1, None, p, s) == EINVAL
    assert L.ldpc_channel_cw_dev(1, 0.1, 1, 0, 8, 1, None, None, s) == EINVAL
    assert L.ldpc_mc_cw_count_dev(p, p, 1, p, None, 8, 1, 4, -1, 0, None, s) == EINVAL
    assert L.ldpc_mc_cw_count_dev(None, p, 1, p, None, 8, 1, 4, -1, 0, cnt.data_ptr(), s) == EINVAL
    assert L.ldpc_mc_cw_count_dev(p, p, 1, p, None, 8, -1, 4, -1, 0, cnt.data_ptr(), s) == EINVAL
    # B = 0 is a no-op, with or without arrays
    assert L.ldpc_encode_batch_dev(h, None, 0, None, s) == 0
    assert L.ldpc_info_bits_dev(1, 0, 8, 0, None, s) == 0
    assert L.ldpc_channel_cw_dev(1, 0.1, 1, 0, 8, 0, None, None, s) == 0
    assert L.ldpc_mc_cw_count_dev(None, None, 1, None, None, 8, 0, 4, -1, 0, cnt.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert (buf == 0x7F).all() and not cnt.any()
    L.ldpc_encoder_destroy(None)


# --------------------------------------------------------------------------- stream order
def test_the_four_entries_in_stream_order(torch):
    """Information bits, encode, codeword channel and count queued on a side stream behind a stall,
    each reading what the call before it wrote: outputs poisoned before the stall and again behind it,
    the counters garbage until they are zeroed behind it."""
    from iib_project_ldpc_codes_amd import _native, decoder
    from iib_project_ldpc_codes_amd.encoder import Encoder
    from tests import stream_util as su
    name, B, iters, seed, first = "r36_1000", 257, 4, 7, 100
    enc = Encoder(eu.tanner(name))
    n, K = enc.n, enc.K
    U = _info_bits(seed, first, B, K)
    x = encode_ref.solve(eu.H(name), enc.info_positions, enc.parity_positions, U)
    llr0 = oracle.channel(oracle.CH_BSC, 0.06, seed, first, n, B)
    llr = np.where(x == 1, -llr0, llr0).astype(np.float32)
    hard = (llr < 0).astype(np.uint8)  # a "decoder" that decides the channel values
    curve = np.zeros((B, iters + 1), np.int64)
    curve[:, 0] = curve[:, -1] = (hard != x).sum(axis=1)
    its = np.full(B, iters, np.int32)
    j = su.Job(torch, "codeword chain")
    d_info = j.output((B, K), torch.uint8, U, "info")
    d_cw = j.output((B, n), torch.uint8, x, "codewords")
    d_llr = j.output((B, n), torch.float32, llr, "llr")
    d_hard, d_its = j.late_input(hard), j.late_input(its)
    cnt = j.accumulator((4 + iters + 1,), torch.int64, gallager_ref.mc_counters(curve, its, -1, 0), "counters")
    j.call(lambda s: enc.info_bits_dev(seed, first, B, out=d_info, stream=s))
    j.call(lambda s: enc.encode_dev(d_info, out=d_cw, stream=s))
    j.call(lambda s: decoder.channel_dev("bsc", 0.06, seed, first, n, B, out=d_llr, stream=s, codewords=d_cw))
    j.call(lambda s: _native.check(_native.lib().ldpc_mc_cw_count_dev(
        d_cw.data_ptr(), d_llr.data_ptr(), 1, d_hard.data_ptr(), d_its.data_ptr(), n, B, iters, -1, 0, cnt.data_ptr(),
        j.stream_ptr(s)), "ldpc_mc_cw_count_dev"))
    for how in ("arg", "current"):
        ended = su.run_jobs(torch, [j], su.side_streams(torch)[0], how)
        assert ended is False, "the stall ended before the calls were enqueued"
        j.check()
