"""What tests/test_gpu_streams.py needs to hold the device entry points to stream order: a bounded
stall, the module's side streams, jobs (one queued call each with its late inputs, sentinel-filled
outputs and the oracle's answer) and the oracle side of the min-sum Monte-Carlo calls at any
iteration count.

The method: stall(stream, seconds) queues a spin of bounded duration on `stream`.  Everything queued
behind it runs late; whatever the library issues on another stream, or does when the call is
enqueued, runs early and meets stale data -- zero-filled inputs that the real ones are copied over
only behind the stall, garbage counters that are zeroed only behind it, outputs that are filled with
the sentinel once before the stall and once more behind it.  The spin is torch.cuda._sleep (a chain of
matmuls without it), calibrated once with two events; it never waits for a host flag, so it cannot
hang the card.

STALL_S: the warm host-side enqueue time of the longest sequence of the file (the twelve calls of
test_queued_calls_on_one_stream with their late copies and fills) was measured at 0.33 ms on an
MI355X host, with the library of the parent commit (this file came without a library change); one
entry with its late inputs takes 0.03 - 0.3 ms.  The stall is 0.25 s, 750 times the longest, so a
loaded host does not outlast it -- and every test that leans on the stall asserts that it was still
running when the last call had been enqueued (run_jobs prints each sequence's enqueue time).
"""
import contextlib
import functools
import os
import time

import numpy as np

from oracle import oracle
from tests import index64_util as u

SENTINEL = 0x7F
STALL_S = 0.25
ALPHA, ITERS = u.ALPHA, u.ITERS
_state = {}


# ------------------------------------------------------------------- streams and the stall
def side_streams(torch):
    """The file's two side streams on the current device, created once."""
    if "streams" not in _state:
        _state["streams"] = (torch.cuda.Stream(), torch.cuda.Stream())
    return _state["streams"]


def _spin(torch, units):
    """`units` of bounded work on the current stream: _sleep cycles, or 1024^2 matmuls in a chain."""
    units = max(1, int(units))
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(units)
        return
    a = _state.setdefault("mm", torch.full((1024, 1024), 1.0 / 1024, device="cuda"))
    b = _state.setdefault("mm_out", torch.empty_like(a))
    for _ in range(units):
        torch.mm(a, a, out=b)


def calibrate(torch):
    """Units of _spin per second on the current device, measured once with two events (the run is
    lengthened until it takes 20 ms, at most three times)."""
    if "rate" in _state:
        return _state["rate"]
    unit = 5_000_000 if hasattr(torch.cuda, "_sleep") else 50
    _spin(torch, unit // 10)
    torch.cuda.synchronize()
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _spin(torch, unit)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 20.0:
            break
        unit *= 8
    assert ms > 0.0
    _state["rate"] = unit / (ms * 1e-3)
    return _state["rate"]


def stall(torch, stream, seconds=STALL_S):
    """Queue a spin of about `seconds` on `stream`; the event recorded right behind it."""
    rate = calibrate(torch)
    with torch.cuda.stream(stream):
        _spin(torch, rate * seconds)
        done = torch.cuda.Event()
        done.record(stream)
    return done


# ------------------------------------------------------------------------------ graphs
@contextlib.contextmanager
def _layout_env(noloc):
    saved = os.environ.pop("LDPC_NO_LOC_LAYOUT", None)
    if noloc:
        os.environ["LDPC_NO_LOC_LAYOUT"] = "1"
    try:
        yield
    finally:
        os.environ.pop("LDPC_NO_LOC_LAYOUT", None)
        if saved is not None:
            os.environ["LDPC_NO_LOC_LAYOUT"] = saved


def graph(spec, noloc=False):
    """(TannerGraph, csr, plan environment) of index64_util.new_graph(spec), its device layout on the
    current device built with or without the local-edge layout; one graph per (spec, noloc), kept."""
    key = ("graph", spec, noloc)
    if key not in _state:
        _state[key] = u.new_graph(spec)
    g = _state[key]
    with _layout_env(noloc):
        g.handle()
    return g, u.fixed_graph(spec)[1], ({"LDPC_NO_LOC_LAYOUT": "1"} if noloc else None)


# -------------------------------------------------------------------------------- jobs
class Job:
    """One queued call: late inputs, outputs and what the oracle says they hold afterwards."""

    def __init__(self, torch, name):
        self.torch, self.name = torch, name
        self.copies, self.zeroed, self.filled, self.wants, self.calls = [], [], [], [], []

    def _dev(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device="cuda")

    def late_input(self, arr):
        """A device tensor of zeros; `arr` is copied over it behind the stall."""
        real = self.torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        dst = self.torch.zeros_like(real)
        self.copies.append((dst, real))
        return dst

    def accumulator(self, shape, dtype, want=None, label=""):
        """A tensor the call adds to (counters, the BEC error rows): sentinel bytes now, zeroed behind
        the stall."""
        t = self._dev(shape, dtype)
        self.zeroed.append(t)
        self.expect(t, want, label)
        return t

    def output(self, shape, dtype, want=None, label=""):
        """A tensor the call writes: sentinel bytes before the stall and again behind it."""
        t = self._dev(shape, dtype)
        self.filled.append(t)
        self.expect(t, want, label)
        return t

    def expect(self, t, want, label=""):
        if want is not None:
            self.wants.append((t, want, label))

    def call(self, fn):
        """fn(stream): enqueue on `stream`, or on the current stream when it is None."""
        self.calls.append(fn)

    def stream_ptr(self, stream):
        return (stream if stream is not None else self.torch.cuda.current_stream()).cuda_stream

    # the steps, in the order run_jobs takes them
    def fill(self):
        for t in self.filled + self.zeroed:
            t.view(self.torch.uint8).fill_(SENTINEL)

    def late(self):
        for dst, real in self.copies:
            dst.copy_(real, non_blocking=True)
        for t in self.zeroed:
            t.zero_()
        for t in self.filled:
            t.view(self.torch.uint8).fill_(SENTINEL)

    def enqueue(self, stream):
        for fn in self.calls:
            fn(stream)

    def check(self):
        for t, want, label in self.wants:
            got = t.cpu().numpy()
            np.testing.assert_array_equal(got.astype(want.dtype) if got.dtype != want.dtype else got, want,
                                          err_msg="%s %s" % (self.name, label))


def run_jobs(torch, jobs, stream, how="arg", stalled=True):
    """Sentinels, [stall,] late inputs and the calls of `jobs` on `stream`, then its synchronisation.
    how: "arg" passes the stream as the calls' stream argument with the default stream current,
    "current" makes it the current stream and passes none.  Returns whether the stall had ended
    when the last call was enqueued (None without a stall)."""
    for j in jobs:
        j.fill()
    torch.cuda.synchronize()
    done = stall(torch, stream) if stalled else None
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        for j in jobs:
            j.late()
        if how == "current":
            for j in jobs:
                j.enqueue(None)
    if how != "current":
        assert how == "arg"
        for j in jobs:
            j.enqueue(stream)
    ended = done.query() if stalled else None
    print("%s: %d calls enqueued in %.2f ms%s" % (jobs[0].name, sum(len(j.calls) for j in jobs),
                                                 1e3 * (time.perf_counter() - t0), "" if stalled else " (no stall)"))
    stream.synchronize()
    return ended


# -------------------------------------------------------------- oracle side: min-sum on the BSC
def minsum_curves(csr, llr, iters, early_stop):
    """index64_util._minsum_curves at any iteration count: per-trial error curves [B][iters + 1] and
    iteration counts of the oracle's flooding min-sum.  A trial that stopped at iteration s keeps its
    decisions, so only the trials still running at t are decoded again with max_iters = t."""
    B = llr.shape[0]
    _, h, its = oracle.bp_decode_batch(csr, llr, iters, 1, alpha=ALPHA, early_stop=early_stop)
    its = its.astype(np.int64)
    curve = np.repeat(h.sum(axis=1, dtype=np.int64)[:, None], iters + 1, axis=1)
    curve[:, 0] = (llr < 0).sum(axis=1)
    for t in range(1, iters):
        idx = np.nonzero(its > t)[0]
        if not idx.size:
            break
        _, ht, _ = oracle.bp_decode_batch(csr, llr[idx], t, 1, alpha=ALPHA, early_stop=early_stop)
        curve[idx, t] = ht.sum(axis=1, dtype=np.int64)
    assert B == curve.shape[0]
    return curve, its


@functools.lru_cache(maxsize=None)
def minsum_trials(spec, p, seed, first, B, iters, early_stop):
    """(curves, iteration counts) of trials first .. first + B - 1 of the min-sum Monte-Carlo on graph
    `spec`, kept."""
    csr = u.fixed_graph(spec)[1]
    llr = u.channel_rows(oracle.CH_BSC, p, seed, u.true_indices(first, B), csr[2].size - 1)
    curve, its = minsum_curves(csr, llr, iters, early_stop)
    curve.setflags(write=False)
    its.setflags(write=False)
    return curve, its


@functools.lru_cache(maxsize=None)
def bsc_llr(spec, p, seed, first, B):
    """The oracle's BSC LLRs of codewords first .. first + B - 1 at the graph's length, kept."""
    n = u.fixed_graph(spec)[1][2].size - 1
    llr = u.channel_rows(oracle.CH_BSC, p, seed, u.true_indices(first, B), n)
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def minsum_decode(spec, p, seed, first, B, iters, early_stop):
    """(post, hard, its) of the oracle's flooding min-sum on bsc_llr(spec, p, seed, first, B), kept."""
    out = oracle.bp_decode_batch(u.fixed_graph(spec)[1], bsc_llr(spec, p, seed, first, B), iters, 1, alpha=ALPHA,
                                 early_stop=early_stop)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------- the two jobs most tests queue
def decode_job(torch, spec, p, seed, first, B, iters, early_stop, noloc=False, want=True, name="decode"):
    """ldpc_bp_decode_batch_dev, min-sum with posteriors, on BSC LLRs that arrive late."""
    from iib_project_ldpc_codes_amd import decoder
    g, _, _ = graph(spec, noloc)
    j = Job(torch, "%s %s B=%d es=%d" % (name, spec, B, early_stop))
    llr = j.late_input(bsc_llr(spec, p, seed, first, B))
    w = minsum_decode(spec, p, seed, first, B, iters, early_stop) if want else (None,) * 3
    post = j.output((B, g.n), torch.float32, w[0], "post")
    hard = j.output((B, g.n), torch.uint8, w[1], "hard")
    its = j.output((B,), torch.int32, w[2], "its")
    j.call(lambda s: decoder.bp_decode_dev(g, llr, iters, "minsum", ALPHA, early_stop, post=post, hard=hard, its=its,
                                           stream=s))
    return j


def mc_job(torch, spec, p, seed, batches, iters, early_stop, stop=0, noloc=False, want=True, name="mc"):
    """ldpc_mc_batch_dev, min-sum on the BSC: the batches [(first, B), ...] queued one behind the
    other into one counters tensor that holds garbage until it is zeroed behind the stall.  The
    expectation is the sequential loop's over the batches' trials in order (consecutive batches: the
    loop over [first, first + sum B))."""
    from iib_project_ldpc_codes_amd.montecarlo import MonteCarlo
    g, _, _ = graph(spec, noloc)
    j = Job(torch, "%s %s %s es=%d stop=%d" % (name, spec, batches, early_stop, stop))
    w = None
    if want:
        parts = [minsum_trials(spec, p, seed, f, B, iters, early_stop) for f, B in batches]
        w = u.counters(np.concatenate([c for c, _ in parts]), np.concatenate([i for _, i in parts]), -1, stop)
    mc = MonteCarlo(g, "bsc", p, iters, algo="minsum", alpha=ALPHA, early_stop=early_stop, seed=seed,
                    batch=max(B for _, B in batches))
    mc.counters = j.accumulator((len(mc.counters),), torch.int64, w, "counters")
    j.mc = mc
    for f, B in batches:
        j.call(lambda s, f=f, B=B: mc.run_batch(f, B, stop, stream=s))
    return j
