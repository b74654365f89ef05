"""Device Monte-Carlo engine (the trial loop of parallel_simulator.py:198-244 / :354-379).

One fused launch per batch: channel (Philox) -> decode -> per-trial error
curve; a second launch applies the expurgation filter
(parallel_simulator_expurgated.py:238) and the sequential 200-frame-error stop
rule (parallel_simulator.py:198) and accumulates int64 counters on the device.

Multi-GPU (one process per GPU, torch.distributed): trials shard by index --
rank r of W runs the batch of trials [(round*W + r)*B, +B); the only collective
is one all-reduce per round of [counter deltas | per-rank frame errors | time
flag] (RCCL over xGMI with backend "nccl", gloo on CPU).  The stop rule is the
reference's sequential one in global trial order: in the round that crosses
stop_frame_errors, ranks before the crossing keep their whole batch, the
crossing rank re-runs its batch (Philox streams are keyed by trial index, so
the re-run is identical) with the in-batch cut at its share of the remaining
frame errors, and later ranks drop theirs -- the counters then equal one
process's `while block_error < 200 and i < num_tests` loop exactly.
"""
import time

import numpy as np

from . import _native
from .decoder import ALGOS, CHANNELS, GALLAGER, _flip_threshold, _quant, _schedule


def device_executor(mc):
    """Batch executor backed by ldpc_mc_batch_dev (mc.schedule "layered": ldpc_mc_layered_batch_dev,
    with mc.quant ldpc_mc_layered_q_batch_dev) on the current HIP device."""
    torch = mc.torch
    entry = "ldpc_mc_layered_batch_dev" if mc.schedule == "layered" else "ldpc_mc_batch_dev"
    if mc.quant is not None:
        entry = "ldpc_mc_layered_q_batch_dev"

    def run(first_cw, B, stop_frame_errors, counters, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream()
        if mc.quant is not None:
            import ctypes as ct
            q = mc.quant.native()
            rc = getattr(_native.lib(), entry)(mc.graph.handle(), mc.channel, mc.param, mc.seed, int(first_cw),
                                               int(B), mc.max_iters, ct.addressof(q), int(mc.early_stop),
                                               mc.expurgation, int(stop_frame_errors), counters.data_ptr(),
                                               s.cuda_stream)
            _native.check(rc, entry)
            return
        rc = getattr(_native.lib(), entry)(mc.graph.handle(), mc.channel, mc.param, mc.seed, int(first_cw),
                                           int(B), mc.max_iters, mc.algo, mc.alpha, int(mc.early_stop),
                                           mc.expurgation, int(stop_frame_errors), counters.data_ptr(),
                                           s.cuda_stream)
        _native.check(rc, entry)
    return run


def gallager_executor(mc):
    """Batch executor of algo="gallager": ldpc_mc_gb_batch_dev (Gallager A/B on the BSC, bit-sliced)."""
    torch = mc.torch

    def run(first_cw, B, stop_frame_errors, counters, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = _native.lib().ldpc_mc_gb_batch_dev(mc.graph.handle(), mc.param, mc.seed, int(first_cw), int(B),
                                                mc.max_iters, mc.flip_threshold, int(mc.early_stop), mc.expurgation,
                                                int(stop_frame_errors), counters.data_ptr(), s.cuda_stream)
        _native.check(rc, "ldpc_mc_gb_batch_dev")
    return run


def codeword_executor(mc):
    """Batch executor of codewords="random": the unfused chain information bits (ldpc_info_bits_dev) ->
    encode (ldpc_encode_batch_dev) -> codeword channel (ldpc_channel_cw_dev) -> the configured decoder's
    device decode entry -> counts against the codeword (ldpc_mc_cw_count_dev).  The soft decoders are
    asked for hard decisions only, so an early-stop decode of a fixed code stays on the local-edge
    kernel; Gallager's received bits are llr < 0.  Buffers are kept per batch size."""
    from . import decoder
    from .encoder import Encoder
    torch = mc.torch
    enc = getattr(mc.graph, "_encoder", None)  # one elimination per graph object, whatever runs share it
    if enc is None:
        enc = mc.graph._encoder = Encoder(mc.graph)
    mc.encoder = enc
    n, K = mc.graph.n, enc.K
    bufs = {}

    def run(first_cw, B, stop_frame_errors, counters, stream=None):
        B = int(B)
        if B <= 0:
            return
        s = stream if stream is not None else torch.cuda.current_stream()
        if B not in bufs:
            u8 = dict(dtype=torch.uint8, device=counters.device)
            bufs[B] = (torch.empty((B, K), **u8), torch.empty((B, n), **u8),
                       torch.empty((B, n), dtype=torch.float32, device=counters.device), torch.empty((B, n), **u8),
                       torch.empty((B,), dtype=torch.int32, device=counters.device))
        info, cw, llr, hard, its = bufs[B]
        with torch.cuda.stream(s):
            enc.info_bits_dev(mc.seed, first_cw, B, out=info, stream=s)
            enc.encode_dev(info, out=cw, stream=s)
            decoder.channel_dev(mc.channel, mc.param, mc.seed, first_cw, n, B, out=llr, stream=s, codewords=cw)
            if mc.gallager:
                bits = (llr < 0).to(torch.uint8)
                decoder.gallager_decode_dev(mc.graph, bits, mc.max_iters, mc.flip_threshold, mc.early_stop, hard=hard,
                                            its=its, stream=s)
            else:
                decoder.bp_decode_dev(mc.graph, llr, mc.max_iters, mc.algo, mc.alpha, mc.early_stop, hard=hard, its=its,
                                      stream=s, want_post=False, schedule=mc.schedule, quant=mc.quant)
        rc = _native.lib().ldpc_mc_cw_count_dev(cw.data_ptr(), llr.data_ptr(), 1, hard.data_ptr(), its.data_ptr(), n, B,
                                                mc.max_iters, mc.expurgation, int(stop_frame_errors),
                                                counters.data_ptr(), s.cuda_stream)
        _native.check(rc, "ldpc_mc_cw_count_dev")
    return run


def rate_match_executor(mc):
    """Batch executor of rate_match=: the unfused chain of codeword_executor with the channel of
    ldpc_channel_rm_dev and the counts of ldpc_mc_rm_count_dev.  BSC / BI-AWGN: [information bits ->
    ratematch.shorten_info -> encode, with codewords="random" only; otherwise the entries get no
    codeword and mean the all-zero one] -> rate-matched channel -> the configured decoder's device
    decode entry -> counts under the description's count mask.  BEC (all-zero codeword): rate-matched
    channel -> a copy of the words -> decoder.bec_decode_dev -> counts of the words still erased.
    Buffers are kept per batch size."""
    from . import decoder, ratematch
    from .encoder import Encoder
    torch = mc.torch
    rm = mc.rate_match
    random = mc.codewords == "random"
    bec = mc.channel == CHANNELS["bec"]
    enc = None
    if random or rm.count == "info":
        enc = getattr(mc.graph, "_encoder", None)  # one elimination per graph object, as codeword_executor
        if enc is None:
            enc = mc.graph._encoder = Encoder(mc.graph)
        mc.encoder = enc
        rm.bind(enc)
    # a shortened parity position: ValueError here, not mid-run
    short = ratematch.shortened_info_index(enc, rm) if random else None
    n, K = mc.graph.n, (enc.K if random else 0)
    bufs, short_dev = {}, {}

    def run(first_cw, B, stop_frame_errors, counters, stream=None):
        B = int(B)
        if B <= 0:
            return
        s = stream if stream is not None else torch.cuda.current_stream()
        if B not in bufs:
            dev = counters.device
            u8 = dict(dtype=torch.uint8, device=dev)
            bufs[B] = (torch.empty((B, K), **u8) if random else None, torch.empty((B, n), **u8) if random else None,
                       torch.empty((B, n), dtype=torch.uint8 if bec else torch.float32, device=dev),
                       torch.empty((B, n), **u8), torch.empty((B,), dtype=torch.int32, device=dev),
                       torch.empty((B, mc.max_iters), dtype=torch.int32, device=dev) if bec else None)
        info, cw, chan, dec, its, err = bufs[B]
        with torch.cuda.stream(s):
            if random:
                enc.info_bits_dev(mc.seed, first_cw, B, out=info, stream=s)
                if short.size:
                    if info.device not in short_dev:  # the index tensor: uploaded once per device
                        short_dev[info.device] = torch.as_tensor(short, device=info.device)
                    ratematch.shorten_info(info, enc, rm, index=short_dev[info.device])
                enc.encode_dev(info, out=cw, stream=s)
            decoder.channel_dev(mc.channel, mc.param, mc.seed, first_cw, n, B, out=chan, stream=s, codewords=cw,
                                rate_match=rm, known_llr=mc.known_llr)
            if bec:
                dec.copy_(chan)
                err.zero_()
                decoder.bec_decode_dev(mc.graph, dec, mc.max_iters, errors=err, its=its, stream=s)
            elif mc.gallager:  # a known position arrives as y = x: llr = +-known_llr
                bits = (chan < 0).to(torch.uint8)
                decoder.gallager_decode_dev(mc.graph, bits, mc.max_iters, mc.flip_threshold, mc.early_stop, hard=dec,
                                            its=its, stream=s)
            else:
                decoder.bp_decode_dev(mc.graph, chan, mc.max_iters, mc.algo, mc.alpha, mc.early_stop, hard=dec, its=its,
                                      stream=s, want_post=False, schedule=mc.schedule, quant=mc.quant)
        rc = _native.lib().ldpc_mc_rm_count_dev(rm.handle(), None if cw is None else cw.data_ptr(), chan.data_ptr(),
                                                0 if bec else 1, dec.data_ptr(), its.data_ptr(), B, mc.max_iters,
                                                mc.expurgation, int(stop_frame_errors), counters.data_ptr(),
                                                s.cuda_stream)
        _native.check(rc, "ldpc_mc_rm_count_dev")
    return run


def fused_codeword_executor(mc):
    """Batch executor of fused=True: [information bits -> ratematch.shorten_info -> encode, with
    codewords="random" only; otherwise no codeword is given and the entry means the all-zero one] ->
    ldpc_mc_layered_q_cw_batch_dev, which draws the channel of the (rate-matched) codeword in the
    fixed-point decoder's kernel and counts every iteration against the codeword under the count
    mask.  Per batch size only the information and codeword buffers are kept."""
    import ctypes as ct
    from . import ratematch
    from .encoder import Encoder
    torch = mc.torch
    rm = mc.rate_match
    random = mc.codewords == "random"
    enc = None
    if random or (rm is not None and rm.count == "info"):
        enc = getattr(mc.graph, "_encoder", None)  # one elimination per graph object, as codeword_executor
        if enc is None:
            enc = mc.graph._encoder = Encoder(mc.graph)
        mc.encoder = enc
        if rm is not None:
            rm.bind(enc)
    # a shortened parity position: ValueError here, not mid-run
    short = ratematch.shortened_info_index(enc, rm) if random and rm is not None else np.zeros(0, np.int64)
    n, K = mc.graph.n, (enc.K if random else 0)
    bufs, short_dev = {}, {}

    def run(first_cw, B, stop_frame_errors, counters, stream=None):
        B = int(B)
        if B <= 0:
            return
        s = stream if stream is not None else torch.cuda.current_stream()
        cw = None
        if random:
            if B not in bufs:
                u8 = dict(dtype=torch.uint8, device=counters.device)
                bufs[B] = (torch.empty((B, K), **u8), torch.empty((B, n), **u8))
            info, cw = bufs[B]
            with torch.cuda.stream(s):
                enc.info_bits_dev(mc.seed, first_cw, B, out=info, stream=s)
                if short.size:
                    if info.device not in short_dev:  # the index tensor: uploaded once per device
                        short_dev[info.device] = torch.as_tensor(short, device=info.device)
                    ratematch.shorten_info(info, enc, rm, index=short_dev[info.device])
                enc.encode_dev(info, out=cw, stream=s)
        q = mc.quant.native()
        rc = _native.lib().ldpc_mc_layered_q_cw_batch_dev(
            mc.graph.handle(), None if rm is None else rm.handle(), None if cw is None else cw.data_ptr(), mc.channel,
            mc.param, mc.known_llr, mc.seed, int(first_cw), B, mc.max_iters, ct.addressof(q), int(mc.early_stop),
            mc.expurgation, int(stop_frame_errors), counters.data_ptr(), s.cuda_stream)
        _native.check(rc, "ldpc_mc_layered_q_cw_batch_dev")
    return run


def fused_check(fused, quant, schedule, channel, codewords, rate_match):
    """ValueError unless fused=True is asked of a configuration that has the fused kernel: the
    fixed-point layered decoder on the BSC or BI-AWGN, with random codewords or a rate-matching
    description (or both)."""
    if not fused:
        return
    if quant is None:
        raise ValueError("fused=True needs quant=: the fused codeword mode is the fixed-point decoders'")
    if schedule != "layered":
        raise ValueError('fused=True needs schedule="layered"')
    if channel not in ("bsc", "awgn"):
        raise ValueError("fused=True is for the BSC and BI-AWGN")
    if codewords != "random" and rate_match is None:
        raise ValueError('fused=True needs codewords="random" or rate_match=: the all-zero, all-transmitted run '
                         "is fused already")


CODEWORDS = ("zero", "random")


def ensemble_executor(mc, n, dv, dc):
    """Batch executor for ensemble mode: trial t decodes on its own random (dv, dc)
    graph t (parallel_simulator.py:198-231 draws a fresh code per trial):
    ldpc_mc_ensemble_batch_dev on the BEC, ldpc_mc_ensemble_soft_batch_dev (mc.algo, mc.alpha,
    mc.early_stop) on the BSC and BI-AWGN."""
    torch = mc.torch

    def run(first_cw, B, stop_frame_errors, counters, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream()
        if mc.channel == CHANNELS["bec"]:
            rc = _native.lib().ldpc_mc_ensemble_batch_dev(n, dv, dc, mc.channel, mc.param, mc.seed, int(first_cw),
                                                          int(B), mc.max_iters, mc.expurgation,
                                                          int(stop_frame_errors), counters.data_ptr(), s.cuda_stream)
            _native.check(rc, "ldpc_mc_ensemble_batch_dev")
            return
        rc = _native.lib().ldpc_mc_ensemble_soft_batch_dev(n, dv, dc, mc.channel, mc.param, mc.algo, mc.alpha,
                                                           int(mc.early_stop), mc.seed, int(first_cw), int(B),
                                                           mc.max_iters, mc.expurgation, int(stop_frame_errors),
                                                           counters.data_ptr(), s.cuda_stream)
        _native.check(rc, "ldpc_mc_ensemble_soft_batch_dev")
    return run


def ml_executor(mc):
    """Batch executor of the "optimal" modes (ldpc_mc_ml_batch_dev): ML decoding of each
    trial's BEC word, plus message passing on the same word when mc.message_passing."""
    torch = mc.torch
    ens = isinstance(mc.graph, _Ensemble)

    def run(first_cw, B, stop_frame_errors, counters, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream()
        g = mc.graph
        rc = _native.lib().ldpc_mc_ml_batch_dev(None if ens else g.handle(), g.n, g.dv if ens else 0,
                                                g.dc if ens else 0, mc.param, mc.seed, int(first_cw), int(B),
                                                mc.max_iters, int(mc.message_passing), mc.expurgation,
                                                int(stop_frame_errors),
                                                counters.data_ptr() if mc.message_passing else None,
                                                mc.counters_ml.data_ptr(), s.cuda_stream)
        _native.check(rc, "ldpc_mc_ml_batch_dev")
    return run


class _Ensemble:
    """Stand-in for a graph in ensemble mode (only n is needed by the counters)."""

    def __init__(self, n, dv, dc):
        self.n, self.dv, self.dc = n, dv, dc


class MonteCarlo:
    """counters = [trials, frame_errors, bit_errors, iterations, curve[0..max_iters]] (int64).

    optimal=True adds ML ("optimal") decoding of every trial's BEC word
    (parallel_simulator.py `optimal`, modes 1/2/4/5): counters_ml = [trials,
    ML frame errors, ML bit errors, 0, ML bit errors]; message_passing=False
    drops the BP decode and the stop rule then counts ML frame errors.

    schedule="layered": the row-serial schedule (decoder.bp_decode_dev) on a fixed code, BSC and
    BI-AWGN, on one rank or sharded; ensemble runs and the ML modes are flooding-only.
    quant=decoder.Quant(...) with schedule="layered" and algo="minsum": the fixed-point layered
    min-sum (alpha is not read).
    algo="gallager": Gallager A (flip_threshold = 0) / B hard-decision decoding of a fixed code on the
    BSC (decoder.gallager_decode_dev), on one rank or sharded; alpha is not read.
    codewords="random": every trial transmits its own random codeword (codeword_executor) instead of
    the all-zero one, and errors are counted against it -- the validation mode for decoders with ties
    (a zero posterior decides 0, which the all-zero shortcut counts as correct).  Fixed codes on the
    BSC and BI-AWGN, every decoder above; unfused, so of the curve only the two ends (channel and
    final errors) are counted.
    rate_match=ratematch.RateMatch(...): the code as its standard sends it (rate_match_executor) --
    punctured positions reach the decoder as erasures / LLRs of +0, shortened ones as known zeros
    (+known_llr), and errors are counted over the description's count mask (ber is per counted bit).
    Fixed codes; every channel (the BEC with the all-zero codeword), every decoder above --
    algo="gallager" only without punctured positions: a hard-decision decoder has no received bit
    there -- and both codewords= modes; codewords="random" needs every shortened position to be an
    information position of the encoder.  Unfused like codewords="random".
    fused=True: the two modes above on the fixed-point decoder in one kernel (fused_codeword_executor)
    -- valid only with quant=, schedule="layered", the BSC or BI-AWGN and at least one of
    codewords="random" / rate_match=.  The counts are the chain's on the same trials, and the curve
    gains its interior: error_curve[t] is the error rate after iteration t over the counted positions
    (error_curve[0] still over the transmitted ones among them)."""

    def __init__(self, graph, channel, param, max_iters, algo="spa", alpha=1.0, early_stop=True,
                 expurgation=-1, seed=0, batch=4096, process_group=None, executor=None, device=None,
                 optimal=False, message_passing=True, schedule="flooding", quant=None, flip_threshold=0,
                 codewords="zero", rate_match=None, known_llr=1024.0, fused=False):
        import torch
        self.torch = torch
        self.graph = graph
        self.channel = CHANNELS[channel]
        self.schedule = _schedule(schedule)
        self.gallager = algo == GALLAGER
        if codewords not in CODEWORDS:
            raise ValueError(f"codewords must be one of {CODEWORDS}, not {codewords!r}")
        self.codewords = codewords
        self.fused = bool(fused)
        fused_check(self.fused, None if self.gallager else quant, self.schedule, channel, codewords, rate_match)
        if codewords == "random":
            if isinstance(graph, _Ensemble):
                raise ValueError('codewords="random" needs a fixed code: a per-trial graph has no encoder')
            if optimal:
                raise ValueError('codewords="random" has no ML mode')
            if self.channel == CHANNELS["bec"]:
                raise ValueError('codewords="random" is for the BSC and BI-AWGN: erasure decoding does not depend '
                                 "on the codeword")
        self.rate_match = rate_match
        self.known_llr = float(known_llr)
        if rate_match is not None:
            if isinstance(graph, _Ensemble):
                raise ValueError("rate_match= needs a fixed code: a description names the variables of one graph")
            if optimal:
                raise ValueError("rate_match= has no ML mode")
            if rate_match.n != graph.n:
                raise ValueError(f"the rate-matching description is of n = {rate_match.n}, the graph of n = {graph.n}")
            if self.gallager and rate_match.n_punct:
                raise ValueError('algo="gallager" cannot decode punctured positions: a hard-decision decoder has no '
                                 "received bit there (known positions are fine)")
            if not (np.isfinite(self.known_llr) and self.known_llr > 0):
                raise ValueError("known_llr must be finite and > 0")
        if self.gallager:
            if self.channel != CHANNELS["bsc"]:
                raise ValueError('algo="gallager" decodes the BSC only')
            if isinstance(graph, _Ensemble):
                raise ValueError('algo="gallager" needs a fixed code (no ensemble form)')
            if self.schedule == "layered" or quant is not None or optimal:
                raise ValueError('algo="gallager" has one schedule and one-bit messages: no layered, quant or ML mode')
            self.flip_threshold = _flip_threshold(flip_threshold)
        elif flip_threshold:
            raise ValueError('flip_threshold belongs to algo="gallager"')
        if self.schedule == "layered":
            if isinstance(graph, _Ensemble):
                raise ValueError("the layered schedule needs a fixed code: no host-built schedule per sampled graph")
            if optimal or self.channel == CHANNELS["bec"]:
                raise ValueError("the layered schedule decodes the BSC and the BI-AWGN channel (no BEC / ML modes)")
        self.param = float(param)
        self.max_iters = int(max_iters)
        self.algo = GALLAGER if self.gallager else ALGOS[algo]
        self.quant = None if self.gallager else _quant(quant, self.schedule, algo)
        self.alpha = float(alpha)
        self.early_stop = bool(early_stop)
        self.expurgation = int(expurgation)
        self.seed = int(seed)
        self.batch = int(batch)
        self.pg = process_group
        dist = torch.distributed
        self.dist = dist if (dist.is_available() and dist.is_initialized()) else None
        self.rank = self.dist.get_rank(process_group) if self.dist else 0
        self.world = self.dist.get_world_size(process_group) if self.dist else 1
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if executor is None else torch.device("cpu")
        self.device = torch.device(device)
        self.counters = torch.zeros(_native.MC_NCOUNT + self.max_iters + 1, dtype=torch.int64, device=self.device)
        self.optimal = bool(optimal)
        self.message_passing = bool(message_passing) or not self.optimal
        self.counters_ml = (torch.zeros(_native.MC_NCOUNT + 1, dtype=torch.int64, device=self.device)
                            if self.optimal else None)
        if self.optimal and self.channel != CHANNELS["bec"]:
            raise ValueError("ML (optimal) decoding is defined for the BEC only")
        if executor is None:
            if self.optimal:
                executor = ml_executor(self)
            elif self.fused:
                executor = fused_codeword_executor(self)
            elif self.rate_match is not None:
                executor = rate_match_executor(self)
            elif self.codewords == "random":
                executor = codeword_executor(self)
            elif self.gallager:
                executor = gallager_executor(self)
            elif isinstance(graph, _Ensemble):
                executor = ensemble_executor(self, graph.n, graph.dv, graph.dc)
            else:
                executor = device_executor(self)
        self.executor = executor
        self.rounds = 0
        self.trial_base = 0   # first trial index of round 0 (a restored run continues here)
        self.trial_base0 = 0  # first trial index of the whole run (snapshot trial range)

    def next_trial(self):
        """Index of the first trial the next round runs (all ranks)."""
        return self.trial_base + self.rounds * self.world * self.batch

    def snapshot(self, g=None):
        """Counter snapshot of the run so far (collective when g is None; see snapshot.py)."""
        from . import snapshot
        return snapshot.from_counters(self, self._global() if g is None else g)

    def restore(self, snap):
        """Continue from a snapshot (snapshot.load(path)); see snapshot.restore."""
        from . import snapshot
        snapshot.restore(self, snap)

    @classmethod
    def ensemble(cls, n, dv, dc, channel, param, max_iters, **kw):
        """Fresh random (dv, dc) code per trial (parallel_simulator.run_simulation on the BEC;
        "bsc" / "awgn" with algo, alpha and early_stop decode on bp_ens_kernel)."""
        return cls(_Ensemble(n, dv, dc), channel, param, max_iters, **kw)

    def run_batch(self, first_cw, B, stop_frame_errors=0, stream=None):
        if stream is None:
            self.executor(first_cw, B, stop_frame_errors, self.counters)
        else:
            self.executor(first_cw, B, stop_frame_errors, self.counters, stream)

    def _global(self):
        c = self.counters.clone()
        if self.optimal:
            c = self.torch.cat([c, self.counters_ml])
        if self.dist is not None and self.world > 1:
            if self.dist.get_backend(self.pg) == "gloo":
                c = c.cpu()
            self.dist.all_reduce(c, group=self.pg)
        return c.cpu().numpy()

    def _frames_trials(self, c, c_ml):
        """(frame errors, trials) the stop rules count: BP counters, or ML ones when
        message passing is off (parallel_simulator.py:226-231 / :240-241)."""
        src = c if self.message_passing else c_ml
        return int(src[1]), int(src[0])

    def _run_delta(self, first_cw, B, stop):
        """Run one batch into fresh zero counters; return (delta, delta_ml)."""
        saved = self.counters, self.counters_ml
        self.counters = self.torch.zeros_like(saved[0])
        self.counters_ml = None if saved[1] is None else self.torch.zeros_like(saved[1])
        try:
            if B > 0:
                self.run_batch(first_cw, B, stop)
            return self.counters, self.counters_ml
        finally:
            self.counters, self.counters_ml = saved

    def _add(self, delta):
        self.counters += delta[0]
        if delta[1] is not None:
            self.counters_ml += delta[1]

    def _allreduce(self, vec):
        if self.dist.get_backend(self.pg) == "gloo":
            vec = vec.cpu()
        self.dist.all_reduce(vec, group=self.pg)
        return vec.cpu().numpy()

    def _batch_size(self, num_tests, trials_before, slot):
        """Trials this rank runs in the round: the reference stops at exactly num_tests
        (parallel_simulator.py:198), so the round's last batches are clamped in trial order."""
        if not num_tests:
            return self.batch
        return int(max(0, min(self.batch, num_tests - trials_before - slot * self.batch)))

    def run(self, num_tests, stop_frame_errors=200, time_limit=None, checkpoint=None, checkpoint_every=1):
        """Run rounds until the global counters reach stop_frame_errors frame errors or
        num_tests trials, or time_limit seconds pass (parallel_simulator.py:198).  Counts
        equal one sequential process's over the same trials; the time limit is decided
        collectively (every rank leaves on the same round).  checkpoint: snapshot path rank 0
        rewrites every checkpoint_every rounds and at the end (snapshot.py)."""
        from . import snapshot
        t0 = time.time()
        g = self._global()
        nc = len(self.counters)
        frames, trials = self._frames_trials(g[:nc], g[nc:])
        while True:
            if stop_frame_errors and frames >= stop_frame_errors:
                break
            if num_tests and trials >= num_tests:
                break
            first_cw = self.trial_base + (self.rounds * self.world + self.rank) * self.batch
            B = self._batch_size(num_tests, trials, self.rank)
            if self.world == 1:
                # one process: the exact sequential stop happens inside the batch
                self.run_batch(first_cw, B, stop_frame_errors)
                self.rounds += 1
                g = self._global()
                expired = time_limit is not None and time.time() - t0 > time_limit
            else:
                delta = self._run_delta(first_cw, B, 0)
                f_mine = self._frames_trials(*[None if d is None else d.cpu() for d in delta])[0]
                onehot = self.torch.zeros(self.world + 1, dtype=self.torch.int64, device=self.device)
                onehot[self.rank] = f_mine
                onehot[self.world] = int(time_limit is not None and time.time() - t0 > time_limit)
                parts = [delta[0]] + ([delta[1]] if delta[1] is not None else []) + [onehot]
                red = self._allreduce(self.torch.cat(parts))
                per_rank = red[-(self.world + 1):-1]
                expired = bool(red[-1])
                if stop_frame_errors and frames + int(per_rank.sum()) >= stop_frame_errors:
                    quota = stop_frame_errors - frames - int(per_rank[:self.rank].sum())
                    if quota <= 0:
                        delta = (self.torch.zeros_like(delta[0]),
                                 None if delta[1] is None else self.torch.zeros_like(delta[1]))
                    elif quota <= f_mine:
                        # the crossing rank: cut at its share, in trial order
                        delta = self._run_delta(first_cw, B, quota)
                    self._add(delta)
                    self.rounds += 1
                    g = self._global()
                    break
                self._add(delta)
                self.rounds += 1
                g = g + red[:len(red) - (self.world + 1)]
            frames, trials = self._frames_trials(g[:nc], g[nc:])
            if checkpoint and self.rank == 0 and self.rounds % max(1, checkpoint_every) == 0:
                snapshot.save(self.snapshot(g), checkpoint)
            if expired:
                break
        if checkpoint and self.rank == 0:
            snapshot.save(self.snapshot(g), checkpoint)
        return self.results(g)

    def results(self, g=None):
        g = self._global() if g is None else g
        n = self.graph.n
        nc = len(self.counters)
        out = {}
        if self.optimal:
            ml = g[nc:]
            t = int(ml[0])
            out = {"ml_num_tests": t, "ml_frame_errors": int(ml[1]), "ml_bit_errors": int(ml[2]),
                   "ml_fer": ml[1] / t if t else float("nan"), "ml_ber": ml[2] / (t * n) if t else float("nan")}
            g = g[:nc]
            if not self.message_passing:
                out.update({"num_tests": t, "raw_counters": g})
                return out
        trials = int(g[0])
        curve = g[_native.MC_NCOUNT:].astype(np.float64)
        if self.codewords == "random" or self.rate_match is not None:
            if not self.fused:  # unfused: only the two ends of the curve
                curve[1:-1] = np.nan
            out = {**out, "codewords": self.codewords, "channel_bit_errors": int(g[_native.MC_NCOUNT])}
        if self.rate_match is not None:  # rates per counted bit; curve[0] counts the transmitted ones among them only
            rm = self.rate_match
            n = int(rm.counts().sum())
            out = {**out, "rate_match": {"n_tx": rm.n_tx, "n_punct": rm.n_punct, "n_known": rm.n_known, "n_count": n}}
        return {**out,
            "num_tests": trials,
            "frame_errors": int(g[1]),
            "bit_errors": int(g[2]),
            "iterations": int(g[3]),
            "fer": g[1] / trials if trials else float("nan"),
            "ber": g[2] / (trials * n) if trials else float("nan"),
            "error_curve": curve / (n * trials) if trials else curve,
            "raw_counters": g,
        }


def mc_run(graph, channel, param, max_iters, devices=(0,), num_tests=0, stop_frame_errors=200, algo="spa",
           alpha=1.0, early_stop=True, expurgation=-1, seed=0, batch=4096, time_limit=None):
    """A whole run over several devices of THIS process through the C ABI's ldpc_mc_run
    (one RCCL all-reduce per round, exact sequential stop rule; no torch.distributed).
    graph: a TannerGraph (fixed code; irregular graphs go through ldpc_mc_run_csr) or
    ``("ensemble", n, dv, dc)`` for a fresh code per trial.  Returns the same dict as
    MonteCarlo.results."""
    import ctypes as ct
    L = _native.lib()
    C = _native.MC_NCOUNT + int(max_iters) + 1
    counters = np.zeros(C, np.int64)
    rounds = np.zeros(1, np.int64)
    devs = np.ascontiguousarray(devices, dtype=np.int32)
    common = (CHANNELS[channel], float(param), ALGOS[algo], float(alpha), int(bool(early_stop)), int(seed),
              int(max_iters), int(expurgation), int(num_tests or 0), int(stop_frame_errors or 0), int(batch),
              float(time_limit or 0.0), devs.ctypes.data, len(devs), counters.ctypes.data, rounds.ctypes.data)
    if isinstance(graph, tuple) and graph[0] == "ensemble":
        _, n, dv, dc = graph
        rc = L.ldpc_mc_run(None, None, n, n - n * dv // dc, dv, dc, *common)
        name = "ldpc_mc_run"
    elif graph.csr is None:
        v2c = np.ascontiguousarray(graph.variable_lookup, np.int32)
        c2v = np.ascontiguousarray(graph.check_lookup, np.int32)
        n = graph.n
        rc = L.ldpc_mc_run(v2c.ctypes.data, c2v.ctypes.data, graph.n, graph.k, graph.dv, graph.dc, *common)
        name = "ldpc_mc_run"
    else:
        cptr, cvar, vptr, vslot = [np.ascontiguousarray(a, np.int32) for a in graph.to_csr()]
        n = graph.n
        rc = L.ldpc_mc_run_csr(cptr.ctypes.data, cvar.ctypes.data, vptr.ctypes.data, vslot.ctypes.data, graph.n,
                               graph.m, *common)
        name = "ldpc_mc_run_csr"
    _native.check(rc, name)
    trials = int(counters[0])
    curve = counters[_native.MC_NCOUNT:].astype(np.float64)
    return {"num_tests": trials, "frame_errors": int(counters[1]), "bit_errors": int(counters[2]),
            "iterations": int(counters[3]), "fer": counters[1] / trials if trials else float("nan"),
            "ber": counters[2] / (trials * n) if trials else float("nan"),
            "error_curve": curve / (n * trials) if trials else curve, "raw_counters": counters,
            "rounds": int(rounds[0]), "devices": [int(d) for d in devs]}
