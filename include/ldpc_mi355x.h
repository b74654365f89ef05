/*
 * ldpc_mi355x.h -- C ABI of libldpc_mi355x.so, the MI355X (gfx950) LDPC
 * belief-propagation engine.
 *
 * Plain C types only (pointers + sizes); no torch / HIP types in signatures.
 * `stream` arguments are hipStream_t passed as void* (NULL = default stream).
 *
 * Every entry point cites the reference interface it replaces or extends
 * (paths relative to roryhighnam/iib_project_ldpc_codes).
 *
 * Return convention for the new entry points: 0 = OK, negative = error
 * (LDPC_E*); ldpc_last_error() returns a human-readable message.  The drop-in
 * message_passing keeps the reference's convention (returns the iteration
 * index) and returns a negative LDPC_E* code on failure.
 *
 * Empty batches: B = 0 is a no-op returning LDPC_OK (after the graph and
 * shape checks); the per-codeword buffers may then be NULL (an empty device
 * tensor's data pointer).  max_iters = 0: BEC words are left as they are with
 * its = 0; soft decoders return the channel LLRs as posteriors.
 *
 * Streams: every `_dev` entry is asynchronous on `stream`.  All its device work --
 * kernels, the memsets that reset the persistent grid's codeword counter and the
 * sampler's search control, the Monte-Carlo cutoff and reduction -- is issued on
 * `stream` and nowhere else, so it is ordered after what the caller queued there
 * before the call (inputs may still be in flight) and before what is queued
 * afterwards; nothing is read or reset when the call is enqueued.  Calls may be
 * queued on one stream without a host synchronisation in between.  Monte-Carlo
 * batches queued into one counters tensor stop exactly: each batch reads
 * counters[1] on the device when it runs, counts the trials up to the one that
 * reaches stop_frame_errors, and later batches add nothing.
 * Scratch (trial rows, message slabs, sampler control, the host forms' staging)
 * lives in grow-only workspaces, one per (device, stream): calls on different
 * streams or devices never share it, and may be issued from different host threads
 * (ldpc_last_error() is per thread).  A workspace grows by freeing and
 * reallocating, which synchronises the whole device: the first call of a larger
 * shape on a (device, stream) blocks the host until the device is idle; calls of
 * shapes already seen there do not block.  ldpc_sample_csr_dev always blocks: it
 * synchronises `stream` before it rewrites the degree structure an earlier launch
 * may still read, and uploads it with a synchronous copy.  The host-pointer forms
 * block until their result is on the host; they stage through the workspace of the
 * NULL stream (message_passing: through its own cached buffers and stream).
 * Because workspaces allocate, the entries cannot be captured into a HIP graph.
 * (tests/test_gpu_streams.py)
 */
#ifndef LDPC_MI355X_H
#define LDPC_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_OK 0
#define LDPC_EINVAL (-1)  /* bad argument / inconsistent graph / value outside {0,1,2} */
#define LDPC_ENODEV (-2)  /* no MI355X visible / HIP runtime error at init */
#define LDPC_EHIP (-3)    /* HIP runtime error during a call */
#define LDPC_ENOMEM (-4)
#define LDPC_EUNSUP (-5)  /* configuration not supported by any kernel */

/* Channels (channels.py:4-26 BEC; BSC and BI-AWGN are new). */
#define LDPC_CH_BEC 0   /* param = erasure probability                          */
#define LDPC_CH_BSC 1   /* param = crossover probability                        */
#define LDPC_CH_AWGN 2  /* param = noise std-dev sigma (BPSK +-1, LLR = 2y/s^2)  */

/* Soft decoding algorithms (no reference counterpart). */
#define LDPC_ALGO_SPA 0      /* sum-product, tanh rule, fp32                     */
#define LDPC_ALGO_MINSUM 1   /* normalized min-sum (alpha), fp32                 */

/* ---------------------------------------------------------------------- */
/* Drop-in                                                                 */
/* ---------------------------------------------------------------------- */
/*
 * Replaces message_passing.c:7 (`int message_passing(int *Mvc, int iterations,
 * int *variable_to_check_list, int *check_to_variable_list, int *errors, int n,
 * int k, int dv, int dc)`), bound by ctypes at parallel_simulator.py:162-164
 * and parallel_simulator_expurgated.py:162-164.  Same symbol, arguments and
 * semantics: Mvc (0/1/2, int32[n]) decoded in place, errors[it] += erasure
 * count per iteration (caller zeroes it), stall skip, returns the break
 * iteration or `iterations`.  Runs one codeword on the current HIP device.
 * Per call: the lists are compared with the last call's (exact memcmp) and the
 * cached device graph reused, or refilled in place for a new code of the same
 * shape; the word and errors[] travel through pinned staging, one copy each
 * way, one stream synchronisation (thread-safe; one cache per process).
 */
int message_passing(int *Mvc, int iterations, int *variable_to_check_list,
                    int *check_to_variable_list, int *errors, int n, int k, int dv, int dc);

/* ---------------------------------------------------------------------- */
/* Tanner graph handle                                                     */
/* ---------------------------------------------------------------------- */
typedef struct ldpc_graph ldpc_graph;

/*
 * Upload a regular graph given in the reference's edge-list format
 * (random_code_generator.c:34-36 check_lookup = check_to_variable_list,
 * int32[(n-k)*dc]; random_code_generator.c:57-62 variable_lookup =
 * variable_to_check_list, int32[n*dv]) to the current device.
 */
int ldpc_graph_create(const int32_t *variable_to_check_list, const int32_t *check_to_variable_list,
                      int n, int k, int dv, int dc, ldpc_graph **out);

/*
 * Upload an irregular graph in CSR slot form (new):
 * check c owns slots [check_ptr[c], check_ptr[c+1]) with check_var[slot] its
 * variable; variable v owns edges [var_ptr[v], var_ptr[v+1]) with var_slot[]
 * naming the slot of each edge.
 */
int ldpc_graph_create_csr(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, ldpc_graph **out);

/*
 * Upload a quasi-cyclic code: H is an mb x nb array of Z x Z blocks, base int32[mb][nb] (row-major)
 * holding -1 for a zero block, otherwise the shift 0 <= s < Z of a circulant permutation.
 *
 * Expansion convention (stated here once; everything else restates it): check r Z + i holds
 * variable c Z + (i + s_rc) mod Z for every non-zero cell (r, c) of block row r, in ascending
 * block-column order -- that order is the check's slot order, so it fixes the "first index" i1 of
 * the fixed-point contract below.  A variable's checks are in ascending check id.
 *
 * LDPC_EINVAL: Z < 1, a shift outside [0, Z), an all-zero block row or block column, a block row
 * with more than 32 non-zero blocks.
 *
 * The graph is an ordinary graph to every decoder, the encoder and the samplers' consumers.  Its
 * layer schedule is not a colouring: a block row has at most one circulant per block column, so
 * its Z checks share no variable, and layer[check] = check / Z (rule "qc/block-row/v1",
 * ldpc_graph_layer_rule).  "(layer, check id) order" in the layered contracts is then plain check
 * order.  The fixed-point layered entries run bp_qc_q_kernel (csrc/bp_qc_q.hip) on it, which forms
 * the variables of a check from the block row's shifts; with LDPC_NO_QC_KERNEL=1 in the
 * environment at creation the graph keeps the block-row schedule and decodes on the table kernels.
 */
int ldpc_graph_create_qc(int mb, int nb, int Z, const int32_t *base, ldpc_graph **out);
/* The name of the rule that gave this graph its layers: "qc/block-row/v1" for a graph of
 * ldpc_graph_create_qc, ldpc_layer_rule() otherwise. */
const char *ldpc_graph_layer_rule(const ldpc_graph *g);

void ldpc_graph_destroy(ldpc_graph *g);
int ldpc_graph_info(const ldpc_graph *g, int32_t *n, int32_t *m, int32_t *num_edges);

/* ---------------------------------------------------------------------- */
/* Batched BEC erasure decoding (message_passing.c:7-82 over B words)     */
/* ---------------------------------------------------------------------- */
/*
 * Host-pointer form: words uint8[B*n] (0/1/2, in/out),
 * errors int32[B*max_iters] (accumulated, as message_passing.c:73),
 * its int32[B] (return value of each message_passing call).
 */
int ldpc_bec_decode_batch(const int32_t *variable_to_check_list, const int32_t *check_to_variable_list,
                          int n, int k, int dv, int dc, uint8_t *words, int B, int max_iters,
                          int32_t *errors, int32_t *its);

/* Device-pointer form on a prepared graph; asynchronous on `stream`. */
int ldpc_bec_decode_batch_dev(const ldpc_graph *g, uint8_t *d_words, int B, int max_iters,
                              int32_t *d_errors, int32_t *d_its, void *stream);

/* ---------------------------------------------------------------------- */
/* Batched soft decoding (new: SURVEY.md 8b-3)                            */
/* ---------------------------------------------------------------------- */
/*
 * llr float[B*n] channel LLRs (log P(0)/P(1)); outputs posterior LLRs
 * post float[B*n] (may be NULL), hard decisions hard uint8[B*n] (may be NULL,
 * 1 where post < 0) and iterations run its int32[B] (may be NULL).
 * early_stop != 0 stops a codeword once its hard decision satisfies every check.
 * With early stop and post == NULL only the stopping iteration's decisions and
 * the iteration counts are produced, which lets the decode run on the
 * local-edge kernel (same decisions and counts as the posterior-returning path).
 */
int ldpc_bp_decode_batch(const int32_t *variable_to_check_list, const int32_t *check_to_variable_list,
                         int n, int k, int dv, int dc, const float *llr, int B, int max_iters,
                         int algo, float alpha, int early_stop, float *post, uint8_t *hard,
                         int32_t *its);

int ldpc_bp_decode_batch_dev(const ldpc_graph *g, const float *d_llr, int B, int max_iters, int algo,
                             float alpha, int early_stop, float *d_post, uint8_t *d_hard,
                             int32_t *d_its, void *stream);

/* ---------------------------------------------------------------------- */
/* On-device channels (channels.py:24-26 new_transmit + BSC / BI-AWGN)     */
/* ---------------------------------------------------------------------- */
/*
 * Channel outputs for the all-zero codeword (parallel_simulator.py:222) of
 * codewords first_cw .. first_cw+B-1, Philox4x32-10 (rocRAND) keyed by seed:
 * BEC writes uint8 0/2 into d_out, BSC / AWGN write float LLRs.
 * Here and in every Monte-Carlo entry below, seed and the trial index
 * first_cw + b are used in full 64-bit width (the low and high words of each
 * are Philox key and counter words): trial t is the same whatever batch it is
 * drawn in, on either side of 2^32 (tests/test_gpu_index64.py).
 */
int ldpc_channel_dev(int channel, float param, uint64_t seed, uint64_t first_cw, int n, int B,
                     void *d_out, void *stream);

/* ---------------------------------------------------------------------- */
/* Monte-Carlo batch (run_simulation trial loop, parallel_simulator.py:198-244) */
/* ---------------------------------------------------------------------- */
/*
 * One fused device batch: B trials first_cw .. first_cw+B-1: channel ->
 * decode -> per-trial statistics.  counters int64[LDPC_MC_NCOUNT + max_iters + 1]
 * on the device, ACCUMULATED (+=):
 *   [0] trials  [1] frame errors  [2] bit errors (residual erasures / wrong bits)
 *   [3] decoding iterations executed  [4..] error curve[0..max_iters]
 *   (BEC: erasures before decoding and after each iteration -- the
 *    `errors` vector of parallel_simulator.py:165 summed as at :227;
 *    soft: wrong hard decisions after each iteration, [4] = channel errors).
 * A trial counts only when its final error count is > expurgation
 * (parallel_simulator_expurgated.py:238); pass -1 for the plain simulator.
 * If stop_frame_errors > 0 the batch honours the sequential stop rule
 * (parallel_simulator.py:198): only trials up to and including the one that
 * brings counters[1] to stop_frame_errors are counted.
 * algo is ignored for BEC (exact erasure decoding, message_passing.c).
 */
#define LDPC_MC_NCOUNT 4
int ldpc_mc_batch_dev(const ldpc_graph *g, int channel, float param, uint64_t seed, uint64_t first_cw,
                      int B, int max_iters, int algo, float alpha, int early_stop, int expurgation,
                      int64_t stop_frame_errors, int64_t *d_counters, void *stream);

/* ---------------------------------------------------------------------- */
/* Gallager A/B: hard-decision decoding on the BSC (csrc/gb.hip)           */
/* ---------------------------------------------------------------------- */
/*
 * Gallager's algorithm A/B, the BSC sibling of message_passing.c: one-bit
 * messages, bit-sliced on the device (a workgroup decodes a plane word of
 * codewords per instruction).  Every value is an integer: the kernels are
 * bit-exact with the text below (tests/gallager_ref.py restates it).
 *
 * Graph: any consistent graph of ldpc_graph_create / ldpc_graph_create_csr,
 * taken slot by slot.  A check that holds a variable twice simply has two slots.
 * The received word is y in {0,1}^n.  There is one bit per edge and direction.
 * The parameter is b (flip threshold), 0 <= b <= 14.
 *
 * For a variable of degree d, the threshold b_d is:
 *   b = 0:  b_d = d - 1 (Gallager A: all the others must disagree).
 *   b >= 1: b_d = min(b, d - 1) (Gallager B).
 *   A variable of degree 1 always sends y_v.
 *
 *   m_vc(e) = y_v for every edge e = (v, c)
 *   iteration t = 1..max_iters:
 *     check c:     m_cv(e_j) = XOR_{k != j} m_vc(e_k)                    (all slots of c)
 *     variable v:  dis_j = m_cv(e_j) ^ y_v,  D = sum_j dis_j             (all d edges of v)
 *                  x_v   = y_v ^ [2 D > d + 1]                           (majority of the d messages and y; a tie keeps y)
 *                  m_vc(e_j) = y_v ^ [D - dis_j >= b_d]   (d >= 2; d = 1: y_v)
 *     early_stop: x satisfies every check -> stop, its = t
 *   hard = x of the last iteration run (max_iters = 0: hard = y, its = 0); without early stop its = max_iters
 *
 * Monte-Carlo uses the all-zero codeword through the BSC stream of
 * ldpc_channel_dev: y_v of trial t is 1 exactly where that stream's LLR is
 * negative.  curve[0] = weight of y, curve[t] = weight of x after iteration t;
 * the tail repeats the stopping iteration's count.  Counters, expurgation and the
 * sequential stop rule are ldpc_mc_batch_dev's; trial index and seed are used in
 * full 64-bit width.
 *
 * Limits: variable degrees <= 15 (the disagreement count is four bit planes),
 * anything larger returns LDPC_EUNSUP; check degree is unbounded.  b outside
 * 0..14, a NULL graph, B < 0 or max_iters < 0 returns LDPC_EINVAL.  If the planes
 * of the graph (one word per slot and per variable, a second per variable under
 * early stop or Monte-Carlo) do not fit LDS at the narrowest plane word (u8), the
 * call returns LDPC_EUNSUP: there is no slab form.
 *
 * d_bits uint8[B*n]: only bit 0 of each byte is read.  d_hard uint8[B*n] and
 * d_its int32[B] may each be NULL.  Both entries are asynchronous on `stream`.
 */
int ldpc_gb_decode_batch_dev(const ldpc_graph *g, const uint8_t *d_bits, int B, int max_iters, int b,
                             int early_stop, uint8_t *d_hard, int32_t *d_its, void *stream);
/* p: the crossover probability, in (0, 0.5).  d_counters: as ldpc_mc_batch_dev. */
int ldpc_mc_gb_batch_dev(const ldpc_graph *g, float p, uint64_t seed, uint64_t first_cw, int B, int max_iters,
                         int b, int early_stop, int expurgation, int64_t stop_frame_errors,
                         int64_t *d_counters, void *stream);

/* ---------------------------------------------------------------------- */
/* Codewords: encoder, information bits, channel, counts (csrc/encode.hip) */
/* ---------------------------------------------------------------------- */
/*
 * Every fused Monte-Carlo entry above transmits the all-zero codeword.  That is
 * exact only for a symmetric decoder that never meets a posterior of exactly
 * zero: hard = post < 0 turns a tie into bit 0, the transmitted bit.  This family
 * is decoder-independent: encode, transmit a codeword, count errors against it.
 *
 * H over GF(2): entry (c, v) is the parity of the number of slots of check c
 * that hold v (a variable a check holds twice cancels, as in the decoders'
 * XOR-over-slots syndrome).  rank = rank(H), K = n - rank: the code's true
 * dimension, which can exceed n - m.  K = 0 is valid (the code is {0}); a variable
 * in no check is an information position.
 *
 * The elimination (ldpc_encode_rule names it; csrc/encode_host.cpp): bit-packed
 * Gauss-Jordan on 64-bit words, columns scanned from n - 1 downward, each pivoting
 * on the lowest unused row that holds a 1.  par_pos[rank]: the pivot columns in
 * pivot order (falling, so parity sits at the high end); info_pos[K]: the other
 * columns, ascending; A: the dense rank x K bit matrix with
 *   x[info_pos[j]] = u[j],   x[par_pos[i]] = XOR_j A[i][j] u[j],
 * packed in uint32 words, row i at A_words + i * ceil(K / 32), bit j of the row =
 * bit (j & 31) of word j >> 5, the padding bits zero.  Deterministic: the same
 * graph gives the same positions and the same A.  Cost about rank^2 n / 128 word
 * operations on the host (seconds at n = 10,000 - 20,000, minutes at n = 64,800).
 *
 * ldpc_encoder_create runs the elimination on the host and uploads the tables to
 * the current device.  ldpc_debug_encoder_build is the same elimination from a
 * CSR check side alone, host-only (no device): A_words, info_pos and par_pos may
 * each be NULL.
 *
 * ldpc_encode_batch_dev: d_info uint8[B*K] (bit 0 of each byte is read; may be
 * NULL when K = 0) -> d_cw uint8[B*n] of 0/1, P = A U over GF(2) bit-sliced
 * (32 codewords per plane word; ldpc_debug_encode_plan).  LDPC_EUNSUP when the
 * information planes of the narrowest tile (4 K bytes) do not fit LDS.
 *
 * ldpc_info_bits_dev: bit j of trial t (= first_cw + row) is bit j & 31 of word
 * (j >> 5) & 3 of the Philox4x32-10 block with counter {j >> 7, 1, t_lo, t_hi}
 * under the channels' key {seed_lo, seed_hi}.  Every channel's second counter
 * word is 0, so the two streams never meet; seed and trial index are used in
 * full 64-bit width, and trial t is the same in any batch.
 *
 * ldpc_channel_cw_dev: the output of ldpc_channel_dev for the same (seed, trial),
 * reflected where the codeword bit x (bit 0 of d_cw's byte) is 1:
 *   BEC: the same erased positions (2), otherwise x;
 *   BSC / AWGN: llr_x = x ? -llr_0 : llr_0, an exact negation.
 * (Physically the noise is (1 - 2x) sigma g: the same law, g being symmetric and
 * independent of x.)  d_cw NULL = the all-zero codeword: ldpc_channel_dev's
 * output bit for bit.  A tie-free symmetric decode of trial t is thus the exact
 * mirror of the fused all-zero decode of trial t.
 *
 * ldpc_mc_cw_count_dev: per trial, channel errors = [llr < 0] != x (chan_is_llr
 * != 0: d_chan float[B*n]; 0: d_chan uint8[B*n] of received bits, bit 0 != x) and
 * final errors = hard != x.  d_counters has ldpc_mc_batch_dev's layout and length
 * and is accumulated: [0]..[3] as there ([3] sums d_its, which may be NULL),
 * curve[0] += channel errors, curve[max_iters] += final errors (max_iters = 0: the
 * one entry takes the final errors).  The curve entries between the two ends are
 * not touched: an unfused decode has no per-iteration view.  Expurgation and the
 * sequential stop rule are ldpc_mc_batch_dev's, on the final errors.
 *
 * Errors: a NULL handle, B < 0, K < 0, n <= 0, a NULL array that is read or
 * written (B > 0), a bad channel parameter: LDPC_EINVAL.  B = 0 is a no-op.  All
 * four device entries are asynchronous on `stream`.
 */
typedef struct ldpc_encoder ldpc_encoder;
int ldpc_encoder_create(const ldpc_graph *g, ldpc_encoder **out);
void ldpc_encoder_destroy(ldpc_encoder *e);
int ldpc_encoder_info(const ldpc_encoder *e, int32_t *n, int32_t *K, int32_t *rank);
int ldpc_encoder_positions(const ldpc_encoder *e, int32_t *info_pos /* K */, int32_t *par_pos /* rank */);
const char *ldpc_encode_rule(void);
int ldpc_debug_encoder_build(const int32_t *check_ptr, const int32_t *check_var, int n, int m, int32_t *rank,
                             int32_t *info_pos, int32_t *par_pos, uint32_t *A_words /* rank * ceil(K/32) */);
int ldpc_encode_batch_dev(const ldpc_encoder *e, const uint8_t *d_info, int B, uint8_t *d_cw, void *stream);
int ldpc_info_bits_dev(uint64_t seed, uint64_t first_cw, int K, int B, uint8_t *d_info, void *stream);
int ldpc_channel_cw_dev(int channel, float param, uint64_t seed, uint64_t first_cw, int n, int B,
                        const uint8_t *d_cw, void *d_out, void *stream);
int ldpc_mc_cw_count_dev(const uint8_t *d_cw, const void *d_chan, int chan_is_llr, const uint8_t *d_hard,
                         const int32_t *d_its, int n, int B, int max_iters, int expurgation,
                         int64_t stop_frame_errors, int64_t *d_counters, void *stream);
/*
 * Host-only: the launch plans of `count` encode calls (csrc/encode_plan.cpp encode_plan), from
 * the shape alone.  calls[i] = {n, K, rank, B} (K + rank = n).  out[i] int64[9] = {threads, W,
 * codewords per workgroup (32 W), grid = ceil(B / (32 W)), dynamic LDS bytes (4 K W), LDS cap
 * (160 KiB - 4 KiB), plane words per parity row (grid W), scratch bytes (4 rank grid W), workgroups
 * of the write pass}: W is the widest of 4, 2, 1 whose planes fit the cap; 1,024 threads when the
 * planes take more than half a CU's LDS, else 256.  A call that fits at no W is a row of zeros
 * named "none", and the entry returns LDPC_EUNSUP after filling every row.  names + 64 i: the
 * display name, encode_parity_kernel<W> or none.
 */
int ldpc_debug_encode_plan(int count, const int32_t *calls, int64_t *out, char *names);

/* ---------------------------------------------------------------------- */
/* Rate matching: punctured and known (shortened) positions               */
/* (csrc/rate_match_host.cpp, csrc/rate_match.hip)                         */
/* ---------------------------------------------------------------------- */
/*
 * The standards' quasi-cyclic codes do not transmit every variable.  A rate-matching
 * description of a length-n code has two parts.
 *
 * The class cls[v] of each variable:
 *   LDPC_RM_TX    transmitted;
 *   LDPC_RM_PUNCT not transmitted, the receiver knows nothing;
 *   LDPC_RM_KNOWN not transmitted, the receiver knows the bit (a shortened position
 *                 is a known position whose bit is 0).
 * The count mask count[v] in {0, 1}: its default (count = NULL) is 1 exactly where
 * cls[v] != LDPC_RM_KNOWN -- a punctured bit is part of the codeword and must be
 * recovered, a known bit is not counted.
 *
 * On the device the description is one byte per variable, bits 0-1 the class, bit 2
 * the count, padded to a multiple of four bytes; a padding byte is LDPC_RM_PUNCT,
 * uncounted (the value 1).  ldpc_debug_rate_match_pack writes these bytes and info =
 * {n, n_tx, n_punct, n_known, n_count} on the host alone (no device; packed and info
 * may each be NULL).  ldpc_rate_match_create validates on the host and uploads once
 * to the current device.
 *
 * ldpc_channel_rm_dev: the output for trial t = first_cw + row, codeword bit x (bit 0
 * of d_cw's byte; d_cw NULL: x = 0 everywhere), position v (d_out uint8[B*n] on the
 * BEC, float[B*n] on the BSC and BI-AWGN):
 *   LDPC_RM_TX:    ldpc_channel_cw_dev's value, bit for bit (one copy of the
 *                  arithmetic serves both).  The Philox stream is indexed by position,
 *                  so puncturing a position changes nothing at any other position.
 *   LDPC_RM_PUNCT: BEC: 2.  BSC / AWGN: +0.0f (the sign bit is clear).
 *   LDPC_RM_KNOWN: BEC: x, never erased.  BSC / AWGN: x ? -known_llr : +known_llr.
 * known_llr must be finite and > 0.  1024 saturates every decoder of this library:
 * the fp32 kernels clamp internally, the quantiser saturates to Q at any scale >= 1/16.
 * Four positions none of which is transmitted cost no Philox block and no Box-Muller
 * pair, only their stores.
 *
 * ldpc_mc_rm_count_dev: per trial a row of max_iters + 1 entries, as
 * ldpc_mc_cw_count_dev's, its interior zero:
 *   row[0]         = channel errors over the positions with class LDPC_RM_TX and
 *                    count = 1: chan_kind 1 (d_chan float[B*n]): [llr < 0] != x;
 *                    chan_kind 2 (d_chan uint8[B*n] of received bits): bit 0 != x;
 *                    chan_kind 0 (d_chan uint8[B*n] of BEC words): word == 2;
 *   row[max_iters] = final errors over the positions with count = 1: d_dec's bit 0 !=
 *                    x, or with chan_kind 0 (d_dec uint8[B*n] of decoded BEC words)
 *                    word == 2.
 * The rows then take ldpc_mc_cw_count_dev's reduction: the counter layout of
 * ldpc_mc_batch_dev, its expurgation and its sequential stop rule, on the final
 * errors.  d_cw NULL: the all-zero codeword.  d_its may be NULL.
 *
 * The rate of the rate-matched code is R = (K - n_known) / n_tx, K the dimension of
 * the mother code.
 *
 * Errors (LDPC_EINVAL): n < 1, a class byte above 2, a count byte above 1, a NULL
 * handle, B < 0 or max_iters < 0, a chan_kind outside 0..2, a bad channel parameter or
 * known_llr, a NULL buffer that would be read or written with B > 0.  B = 0 is a
 * no-op.  Both device entries are asynchronous on `stream` and take the workspace and
 * its lock as ldpc_channel_cw_dev and ldpc_mc_cw_count_dev do.
 */
#define LDPC_RM_TX 0
#define LDPC_RM_PUNCT 1
#define LDPC_RM_KNOWN 2
typedef struct ldpc_rate_match ldpc_rate_match;
int ldpc_rate_match_create(int n, const uint8_t *cls /* host [n] */, const uint8_t *count /* host [n], NULL = default */,
                           ldpc_rate_match **out);
void ldpc_rate_match_destroy(ldpc_rate_match *rm);
int ldpc_rate_match_info(const ldpc_rate_match *rm, int32_t *n, int32_t *n_tx, int32_t *n_punct, int32_t *n_known,
                         int32_t *n_count);
int ldpc_channel_rm_dev(const ldpc_rate_match *rm, int channel, float param, float known_llr, uint64_t seed,
                        uint64_t first_cw, int B, const uint8_t *d_cw /* NULL = all-zero */, void *d_out, void *stream);
int ldpc_mc_rm_count_dev(const ldpc_rate_match *rm, const uint8_t *d_cw /* NULL = all-zero */, const void *d_chan,
                         int chan_kind /* 0 BEC words, 1 float LLRs, 2 received bits */,
                         const uint8_t *d_dec /* hard bits, or BEC words when chan_kind = 0 */,
                         const int32_t *d_its /* may be NULL */, int B, int max_iters, int expurgation,
                         int64_t stop_frame_errors, int64_t *d_counters, void *stream);
int ldpc_debug_rate_match_pack(int n, const uint8_t *cls, const uint8_t *count, uint8_t *packed /* [4*ceil(n/4)] */,
                               int32_t *info /* [5] */);

/* ---------------------------------------------------------------------- */
/* Layered (row-serial) schedule on a fixed code (csrc/bp_layer.hip)       */
/* ---------------------------------------------------------------------- */
/*
 * The schedule of hardware LDPC decoders ("turbo-decoding message passing"): the
 * checks are split into layers 0..L-1, no two checks of a layer sharing a variable
 * (ldpc_debug_layer_schedule), and every check works on posteriors the checks before
 * it have already updated.  With P = posteriors float[n], R = check->variable
 * messages float[E]:
 *   P[v] = llr[v], R[e] = +0
 *   iteration t = 1..max_iters:
 *     for each check c in (layer, id) order, slots e_j, variables v_j:
 *       x_j = P[v_j] - R[e_j];  r = check rule on x;  P[v_j] = x_j + r_j;  R[e_j] = r_j
 *     hard[v] = P[v] < 0;  early_stop: hard satisfies every check -> stop, its = t
 * (fp32, no contraction; min-sum is bit-exact with this text, the checks of a layer
 * being independent).  Arguments, outputs, the NULL rules, B = 0 and max_iters = 0 as
 * ldpc_bp_decode_batch_dev.  The schedule exists for every consistent graph with check
 * degrees 1..32 in which no check holds a variable twice; any other graph: LDPC_EUNSUP.
 */
int ldpc_bp_layered_decode_batch_dev(const ldpc_graph *g, const float *d_llr, int B, int max_iters, int algo,
                                     float alpha, int early_stop, float *d_post, uint8_t *d_hard,
                                     int32_t *d_its, void *stream);
/*
 * ldpc_mc_batch_dev on the layered schedule, BSC and BI-AWGN (LDPC_CH_BEC:
 * LDPC_EINVAL): curve[0] = channel errors, curve[t] = posteriors < 0 after
 * iteration t, repeated after a stop; counters, expurgation and the sequential
 * stop rule exactly as there.
 */
int ldpc_mc_layered_batch_dev(const ldpc_graph *g, int channel, float param, uint64_t seed, uint64_t first_cw,
                              int B, int max_iters, int algo, float alpha, int early_stop, int expurgation,
                              int64_t stop_frame_errors, int64_t *d_counters, void *stream);

/* ---------------------------------------------------------------------- */
/* Fixed-point layered min-sum with compressed check records               */
/* (csrc/bp_layer_q.hip)                                                    */
/* ---------------------------------------------------------------------- */
/*
 * The layered schedule above as hardware decoders run it: q-bit messages, slightly wider
 * saturating posteriors, and per check a compressed record (two minima, the index of the
 * first, the signs) instead of one message per edge.  Parameters: ldpc_quant, with
 * Q = 2^(msg_bits-1) - 1 and Pmax = 2^(post_bits-1) - 1.
 *
 * A parameter set is valid when all of these hold; anything else returns LDPC_EINVAL:
 *   2 <= msg_bits <= 7
 *   msg_bits <= post_bits <= 8
 *   1 <= norm8 <= 8
 *   0 <= offset <= Q
 *   scale finite and > 0
 *
 * All arithmetic is in integers except the one fp32 product of the channel quantiser.
 *
 *   c[v]  = rint_half_even(clamp(llr[v] * scale, -Q, +Q))      (fp32 product, no contraction; NaN -> 0)
 *   P[v]  = c[v];  R[e] = 0
 *   iteration t = 1..max_iters, checks in (layer, check id) order of the existing layer schedule,
 *     slots e_j, variables v_j of the check:
 *       x_j  = P[v_j] - R[e_j]                                  (not saturated; |x_j| <= Pmax + Q)
 *       a_j  = min(|x_j|, Q);  s_j = (x_j < 0)                  (0 counts as positive)
 *       m1 = min a_j, i1 = first index reaching it, m2 = min over j != i1 (degree 1: m2 = Q)
 *       f(m) = max(((m * norm8) >> 3) - offset, 0)
 *       |r_j| = f(m2) if j == i1 else f(m1);  r_j negative iff (XOR of all s) ^ s_j, and |r_j| > 0
 *       P[v_j] = clamp(x_j + r_j, -Pmax, +Pmax);  R[e_j] = r_j
 *     hard[v] = P[v] < 0;  early_stop: hard satisfies every check -> stop, its = t
 *
 * Outputs are post int8[B][n] (the integers P; NULL allowed), hard uint8[B][n] (NULL allowed)
 * and its int32[B].  max_iters = 0 returns c and c < 0, with its = 0.  B = 0, the NULL rules
 * and streams behave as ldpc_bp_layered_decode_batch_dev.  A graph without a layer schedule
 * returns LDPC_EUNSUP.  A graph whose block does not fit LDS (ldpc_debug_layer_q_plan) returns
 * LDPC_EUNSUP.
 *
 * R is written per edge above only to define the result.  The record (f(m1), f(m2), i1, sign
 * bits of r) reproduces it exactly.  The kernel stores the record, never R.
 */
typedef struct ldpc_quant {
    float scale;
    int32_t msg_bits, post_bits, norm8, offset;
} ldpc_quant;
int ldpc_bp_layered_q_decode_batch_dev(const ldpc_graph *g, const float *d_llr, int B, int max_iters,
                                       const ldpc_quant *q, int early_stop, int8_t *d_post, uint8_t *d_hard,
                                       int32_t *d_its, void *stream);
/*
 * ldpc_mc_layered_batch_dev on the fixed-point decoder (the device channel's LLR goes through the
 * quantiser): curve[0] = c < 0, curve[t] = P < 0 after iteration t, repeated after a stop;
 * counters, expurgation and the sequential stop rule exactly as there.  LDPC_CH_BEC: LDPC_EINVAL.
 */
int ldpc_mc_layered_q_batch_dev(const ldpc_graph *g, int channel, float param, uint64_t seed, uint64_t first_cw,
                                int B, int max_iters, const ldpc_quant *q, int early_stop, int expurgation,
                                int64_t stop_frame_errors, int64_t *d_counters, void *stream);
/*
 * The fused Monte-Carlo batch above on a transmitted codeword and a rate-matched word: the
 * channel is drawn in the decoder's kernel and every iteration is counted against the codeword
 * under the count mask.  rm NULL: every position transmitted and counted; d_cw uint8[B][n], bit 0
 * of each byte, NULL: the all-zero codeword.  For trial t = first_cw + row and position v, with
 * codeword bit x_v:
 *   channel  llr_v is exactly what ldpc_channel_rm_dev writes for (seed, t, v): the reflected stream
 *            where the class is LDPC_RM_TX, +0.0f where LDPC_RM_PUNCT, x_v ? -known_llr : +known_llr
 *            where LDPC_RM_KNOWN.  With rm NULL it is ldpc_channel_cw_dev's value, with d_cw NULL as
 *            well ldpc_channel_dev's.  A group of four positions 4g .. 4g + 3 without a transmitted
 *            one draws no Philox block.
 *   decode   c_v = quantise(llr_v); then ldpc_bp_layered_q_decode_batch_dev's text, unchanged.  Early
 *            stop tests the syndrome of the decisions (the transmitted word is a codeword).
 *   row      max_iters + 1 entries per trial:
 *              row[0] = #{v : class TX, count = 1, [llr_v < 0] != x_v}  (ldpc_mc_rm_count_dev's rule,
 *                       on the sign of the float),
 *              row[t] = #{v : count = 1, [P_v < 0] != x_v} after iteration t, repeated after a stop;
 *            max_iters = 0: the one entry is the final count, of the quantised channel values
 *            c_v.  its as in ldpc_mc_layered_q_batch_dev.
 *   reduce   the rows go through ldpc_mc_batch_dev's reduction: counter layout, expurgation and
 *            the sequential stop rule are its.
 * So: counters [0..3], curve[0] and curve[max_iters] equal those of the unfused chain
 * (ldpc_channel_rm_dev / ldpc_channel_cw_dev, ldpc_bp_layered_q_decode_batch_dev,
 * ldpc_mc_rm_count_dev / ldpc_mc_cw_count_dev) on the same trials; the interior of the curve is what
 * the chain cannot give.  With rm and d_cw both NULL everything except curve[0] equals
 * ldpc_mc_layered_q_batch_dev's output: that entry counts c_v < 0 there and llr_v < 0 here, which
 * differ wherever a small negative LLR quantises to 0.
 * LDPC_EINVAL: LDPC_CH_BEC, a bad q or channel parameter, known_llr not finite and > 0 when rm has
 * a LDPC_RM_KNOWN position, an rm of another n, NULL g / q / d_counters, B < 0 or max_iters < 0.
 * LDPC_EUNSUP: a graph without a layer schedule, or whose block with the codeword's bit plane
 * (ldpc_debug_layer_q_cw_plan) does not fit LDS.  B = 0 is a no-op.  Asynchronous on `stream`.
 */
int ldpc_mc_layered_q_cw_batch_dev(const ldpc_graph *g, const ldpc_rate_match *rm, const uint8_t *d_cw, int channel,
                                   float param, float known_llr, uint64_t seed, uint64_t first_cw, int B,
                                   int max_iters, const ldpc_quant *q, int early_stop, int expurgation,
                                   int64_t stop_frame_errors, int64_t *d_counters, void *stream);

/* ---------------------------------------------------------------------- */
/* Whole Monte-Carlo run over several devices of one process */
/* ---------------------------------------------------------------------- */
/*
 * Replaces the trial loop of run_simulation / run_simulation_fixed_ldpc
 * (parallel_simulator.py:198-244, :354-379; parallel_simulator_expurgated.py
 * :200-256) together with the reference's multi-process fan-out
 * (parallel_simulator.py:403-445) and CSV merge (tools/combine_data.py:64-95):
 * one call runs `while frame_errors < stop_frame_errors and trials < num_tests`
 * (either limit <= 0 = none; time_limit_s <= 0 = none, else checked after each
 * round) over devices[0..ndev) (HIP ordinals, each listed once).  Device slot r
 * of round R decodes trials [(R*ndev + r)*batch, +batch); the counters of each
 * round are summed with ONE ncclAllReduce over the devices (RCCL,
 * ncclCommInitAll, loaded from librccl.so.1 at first use).  The stop rule is
 * applied exactly in global trial order, so the result equals one sequential
 * process over the same trials whatever ndev is.
 *   Graph: the reference's edge lists (fixed code, built on every device) -- or
 *   both lists NULL for ensemble mode (a fresh random (dv, dc) code per trial,
 *   parallel_simulator.py:215: every channel, through
 *   ldpc_mc_ensemble_soft_batch_dev); ldpc_mc_run_csr takes a CSR graph
 *   (irregular codes).
 *   counters (host) int64[LDPC_MC_NCOUNT + max_iters + 1], layout as
 *   ldpc_mc_batch_dev, overwritten; rounds (may be NULL) = rounds run.
 */
int ldpc_mc_run(const int32_t *variable_to_check_list, const int32_t *check_to_variable_list, int n, int k,
                int dv, int dc, int channel, float param, int algo, float alpha, int early_stop, uint64_t seed,
                int max_iters, int expurgation, int64_t num_tests, int64_t stop_frame_errors, int batch,
                double time_limit_s, const int *devices, int ndev, int64_t *counters, int64_t *rounds);
int ldpc_mc_run_csr(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                    const int32_t *var_slot, int n, int m, int channel, float param, int algo, float alpha,
                    int early_stop, uint64_t seed, int max_iters, int expurgation, int64_t num_tests,
                    int64_t stop_frame_errors, int batch, double time_limit_s, const int *devices, int ndev,
                    int64_t *counters, int64_t *rounds);

/* ---------------------------------------------------------------------- */
/* Random regular graphs + ensemble Monte-Carlo           */
/* ---------------------------------------------------------------------- */
/*
 * Replaces generate_random_code (random_code_generator.c:21-67, called per
 * trial at parallel_simulator.py:215 / parallel_simulator_expurgated.py:221-223):
 * G graphs first_graph .. first_graph+G-1 of the (dv, dc) configuration model
 * with whole-graph redraw while any check holds a variable twice, in the
 * reference's edge-list format: check_lookup int32[G][n*dv] (variables of check
 * c at [c*dc, c*dc+dc)), variable_lookup int32[G][n*dv] (checks of each variable,
 * ascending).  Counter-based (Philox, key = seed): graph g is the same whatever
 * G / first_graph batch it is drawn in; seed and the graph index first_graph + g
 * are used in full 64-bit width, here and in the CSR form below (an ensemble
 * trial t draws graph t).  attempts int32[G] (may be NULL): number
 * of permutations drawn for each graph.  The dense parity-check matrix is never
 * built.
 */
int ldpc_sample_regular_dev(int n, int dv, int dc, uint64_t seed, uint64_t first_graph, int G,
                            int32_t *d_check_lookup, int32_t *d_variable_lookup, int32_t *d_attempts,
                            void *stream);
int ldpc_sample_regular(int n, int dv, int dc, uint64_t seed, uint64_t first_graph, int G,
                        int32_t *check_lookup, int32_t *variable_lookup, int32_t *attempts);

/*
 * Irregular form (the same law for any degree structure): n
 * variables with var_ptr[v+1]-var_ptr[v] sockets each, m checks with
 * check_ptr[c+1]-check_ptr[c] slots each (host arrays, var_ptr[n] ==
 * check_ptr[m] == E); a uniformly random socket->slot matching, redrawn whole
 * while any check holds a variable twice.  Output per graph g (row-major):
 * check_var int32[G][E] (variable of each slot, check-major) and var_slot
 * int32[G][E] (for variable v, entries var_ptr[v].. = its slots ascending) --
 * the ldpc_graph_create_csr layout.  Same generator as ldpc_sample_regular
 * (which is this with var_ptr = v*dv, check_ptr = c*dc, var_slot -> check ids).
 */
int ldpc_sample_csr_dev(int n, int m, const int32_t *var_ptr, const int32_t *check_ptr, uint64_t seed,
                        uint64_t first_graph, int G, int32_t *d_check_var, int32_t *d_var_slot, int32_t *d_attempts,
                        void *stream);
int ldpc_sample_csr(int n, int m, const int32_t *var_ptr, const int32_t *check_ptr, uint64_t seed,
                    uint64_t first_graph, int G, int32_t *check_var, int32_t *var_slot, int32_t *attempts);

/*
 * Ensemble BEC Monte-Carlo batch (run_simulation, parallel_simulator.py:168-272;
 * expurgated :169-285): trial t = first_cw + b draws graph t and channel word t,
 * decodes with message_passing semantics and accumulates counters exactly as
 * ldpc_mc_batch_dev (expurgation, sequential stop rule).  channel must be
 * LDPC_CH_BEC; the other channels: ldpc_mc_ensemble_soft_batch_dev.
 */
int ldpc_mc_ensemble_batch_dev(int n, int dv, int dc, int channel, float param, uint64_t seed,
                               uint64_t first_cw, int B, int max_iters, int expurgation,
                               int64_t stop_frame_errors, int64_t *d_counters, void *stream);

/*
 * Soft decoding over the ensemble (new; the soft twin of ldpc_ml_ensemble_decode_dev):
 * word b of d_llr float[B*n] is decoded on graph b of d_check_lookup /
 * d_variable_lookup, int32[B][n*dv] each in the ldpc_sample_regular_dev output
 * layout.  Precondition: the lists are as the sampler writes them -- a simple
 * (dv, dc)-regular graph, both lists naming the same edges, each variable's checks
 * ascending; other lists give undefined decisions (never an access outside the
 * buffers).  The lists are only read.  Outputs, the NULL rules, B = 0, max_iters = 0
 * and early_stop as ldpc_bp_decode_batch_dev; one workgroup per word builds the
 * graph's cross index itself (csrc/bp_ens.hip), so no host-side graph is prepared.
 * Check degrees above 32: LDPC_EUNSUP.
 */
int ldpc_bp_ensemble_decode_dev(int n, int dv, int dc, const int32_t *d_check_lookup,
                                const int32_t *d_variable_lookup, const float *d_llr, int B, int max_iters,
                                int algo, float alpha, int early_stop, float *d_post, uint8_t *d_hard,
                                int32_t *d_its, void *stream);

/*
 * Ensemble Monte-Carlo batch on any channel: trial t = first_cw + b draws graph t
 * (ldpc_sample_regular law, key = seed) and channel word t, decodes with algo /
 * alpha / early_stop (the fused BSC / BI-AWGN channel of ldpc_mc_batch_dev) and
 * accumulates counters exactly as ldpc_mc_batch_dev (expurgation, sequential stop
 * rule).  LDPC_CH_BEC forwards to ldpc_mc_ensemble_batch_dev (algo, alpha and
 * early_stop are then ignored).
 */
int ldpc_mc_ensemble_soft_batch_dev(int n, int dv, int dc, int channel, float param, int algo, float alpha,
                                    int early_stop, uint64_t seed, uint64_t first_cw, int B, int max_iters,
                                    int expurgation, int64_t stop_frame_errors, int64_t *d_counters,
                                    void *stream);

/* ---------------------------------------------------------------------- */
/* ML ("optimal") erasure decoding                        */
/* ---------------------------------------------------------------------- */
/*
 * Replaces regular_LDPC_code.optimal_decode (parallel_simulator.py:60-129;
 * expurgated :60-129) together with the ml_decode set-up it calls through ctypes
 * (ml_decoder.c:7-36, bound at parallel_simulator.py:83-84) and the GF(2)
 * row_reduce of the galois package (:89-91, :108).  Words are uint8 [B][n]:
 * 0/1 known bits, 2 erasures (any other non-zero value is a known 1 and is
 * returned as given).  Output: the decoded words, 2 where an unknown was given up
 * by the reference's loop (first non-pivot column dropped with all its checks,
 * system reduced again); words with no erasure or more erasures than n-k are
 * returned unchanged.  unsolved int32 [B] = the number of 2s in each output word
 * (the reference's optimal_error_count, :235).  d_out may alias d_words.
 * Needs m = n-k <= 1000 (the range in which the reference's 1000-unknown cap,
 * :96, never binds) and n <= 32767; otherwise LDPC_EINVAL.
 */
int ldpc_ml_decode_batch_dev(const ldpc_graph *g, const uint8_t *d_words, int B, uint8_t *d_out,
                             int32_t *d_unsolved, void *stream);
int ldpc_ml_decode_batch(const ldpc_graph *g, const uint8_t *words, int B, uint8_t *out, int32_t *unsolved);

/* Ensemble form: word b is decoded on graph b of d_check_lookup int32[B][n*dv]
 * (the ldpc_sample_regular_dev output layout). */
int ldpc_ml_ensemble_decode_dev(int n, int dv, int dc, const int32_t *d_check_lookup, const uint8_t *d_words, int B,
                                uint8_t *d_out, int32_t *d_unsolved, void *stream);

/*
 * Monte-Carlo batch of the "optimal" modes 1/2/4/5 (parallel_simulator.py:
 * 168-272 / 274-401, `optimal` = True): BEC(eps) channel word t = first_cw + b,
 * ML-decoded; with message_passing != 0 the same word is also BEC-decoded for
 * max_iters iterations (modes 2/5).  g == NULL: ensemble mode, trial t decodes on
 * graph t of the (n, dv, dc) sampler (ldpc_sample_regular law, key = seed);
 * otherwise n/dv/dc are ignored.  d_counters_ml int64[LDPC_MC_NCOUNT + 1] =
 * [trials, ML frame errors, ML bit errors (# of 2s), 0, # of 2s];
 * d_counters_mp int64[LDPC_MC_NCOUNT + max_iters + 1] as ldpc_mc_batch_dev
 * (expurgation applies to it only, as parallel_simulator_expurgated.py:238-245).
 * The sequential stop rule counts message-passing frame errors when
 * message_passing != 0, ML frame errors otherwise (parallel_simulator.py:186-242).
 */
int ldpc_mc_ml_batch_dev(const ldpc_graph *g, int n, int dv, int dc, float eps, uint64_t seed, uint64_t first_cw,
                         int B, int max_iters, int message_passing, int expurgation, int64_t stop_frame_errors,
                         int64_t *d_counters_mp, int64_t *d_counters_ml, void *stream);

/* ---------------------------------------------------------------------- */
/* Diagnostics (host only, no GPU needed)                                  */
/* ---------------------------------------------------------------------- */
/*
 * The conflict-aware lane layout the LDS-resident soft kernel uses for this
 * graph: *T threads x *VPT variables per thread; lane_var int32[T*VPT]
 * (-1 = padding), lane_slot int32[T*VPT*dv].  Pass NULL arrays to query T/VPT.
 */
int ldpc_debug_lane_layout(const int32_t *variable_to_check_list, const int32_t *check_to_variable_list,
                           int n, int k, int dv, int dc, int32_t *T, int32_t *VPT, int32_t *lane_var,
                           int32_t *lane_slot);

/*
 * The irregular kernel's layout for a consistent CSR graph (ldpc_graph_create_csr
 * arguments): shape[5] = {VPT, KC (check rows of 1024), DC (slots per check),
 * S (positions in LDS), P (positions in all)}; lane int32[3][1024*VPT] (variable
 * id or -1, positions of edges 0|1<<16 and 2|3<<16, 0xFFFF = none); cdeg
 * int32[2][1024] (check degrees, 4 bits per row).  Returns LDPC_EUNSUP when the
 * graph is outside the kernel's range.  Pass NULL arrays to query the shape.
 */
int ldpc_debug_irr_layout(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, int32_t *shape, int32_t *lane, int32_t *cdeg);

/*
 * Host-only: the local-edge layout of bp_loc_kernel for a CSR graph (no device
 * needed; tests / diagnostics).  shape: int32[24] = {T, KP, DVN, P, words, classes,
 * bank-conflict cost, cls_q[5], cls_d[4], cls_w[5], DVN0 | ABS0 << 8, DVN1 | ABS1 << 8}; var: int32[2*KP*2*T] variable
 * ids, pos: int32[2*KP*max(DVN,1)*T] packed LDS words, info: int32[2*KP*T] (see
 * ldpc_graph::loc_* in csrc/ldpc_internal.hpp).  NULL arrays: shape only.  Returns
 * LDPC_EUNSUP when the graph has no such layout.
 */
int ldpc_debug_loc_layout(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, int T, int32_t *shape, int32_t *var, int32_t *pos,
                          int32_t *info);

/*
 * The chained local-edge layout that fixed-count sum-product decodes of (3,6) codes run on (host
 * only): the plain T = 512 layout with each thread's five .x (and five .y) checks on a path
 * whose link variables keep a second edge in registers (csrc/loc_layout.cpp).  shape: int32[6] =
 * {Tq, KP, chain links per thread, words, bank-conflict cost, T}; var, pos, info: as
 * ldpc_debug_loc_layout's at T = 512 with DVN = 2; chk: int32[2*KP*T], the check at pair slot k,
 * half h of thread t at (2k + h)*T + t (-1: none).  NULL arrays: shape only.  Returns
 * LDPC_EUNSUP when the graph has no chained layout.
 */
int ldpc_debug_loc_chain_layout(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                                const int32_t *var_slot, int n, int m, int32_t *shape, int32_t *var, int32_t *pos,
                                int32_t *info, int32_t *chk);

/*
 * Host-only: the launch plans of `count` soft-decoding calls on one CSR graph (csrc/bp_plan.cpp
 * bp_plan), from the host layouts alone; cus: compute units of the device planned for.
 * calls[i] = {B, iters, algo, early_stop, mc, want_post}; out[i] int64[9] = {path, threads,
 * grid, LDS bytes, lds_slots, persistent, slab bytes, counter offset (-1: none), scratch
 * bytes}; names + 64 i: the kernel's display name.
 */
int ldpc_debug_bp_plan(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                       const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus, int64_t *out,
                       char *names);

/*
 * Host-only: ldpc_debug_bp_plan with the calls' device pointers -- their addresses alone, nothing is
 * read through them.  calls[i] int64[9] = {B, iters, algo, early_stop, mc, llr, post, hard, narrow}
 * (post = 0: no posteriors asked for; narrow: LDPC_NO_WIDE_IO=1); out[i] int64[11] =
 * ldpc_debug_bp_plan's nine, then wide_io (1: bp_loc_kernel's fixed-count decode moves its rows 16
 * bytes at a time: llr and post 16-byte aligned, hard 4-byte aligned, a null one counts as aligned)
 * and the words of bp_loc_kernel's message LDS (at least n + 4: the spare words behind the staged
 * rows; 0 on another path).
 */
int ldpc_debug_bp_plan_io(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, int count, const int64_t *calls, int cus, int64_t *out,
                          char *names);

/*
 * Host-only: the launch width of ldpc_debug_bp_plan's calls (same calls[i] int32[6]); out[i] int64 =
 * the threads a workgroup is launched with.  The fixed-count sum-product call on a graph with a
 * chained layout launches that layout's Tq threads (n / 20: only they own checks and variables;
 * `threads` stays 512, its instantiation's shape and the stride of its tables); every other call
 * launches the plan's `threads`.
 */
int ldpc_debug_bp_plan_width(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                             const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus,
                             int64_t *out);

/*
 * Host-only: the compile-time width of the same calls; out[i] int64 = Tq when the call is the
 * fixed-count sum-product decode on a chained layout whose Tq has an instantiation of its own
 * (bp_loc_chain_kernel with Tq a template argument: 500, n = 10,000), 0 for every other call and width,
 * and for every call under LDPC_NO_LOC_TQ=1 (read when the graph's layouts are built).
 */
int ldpc_debug_bp_plan_tq(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus,
                          int64_t *out);

/*
 * Test entry: ldpc_bp_decode_batch_dev's fixed-count sum-product decode (B > 0) on a graph with a
 * chained layout, launched from its own plan with the plan's compile-time width replaced by tq.
 * tq = 0 runs the generic instantiation; a tq that is not the graph's Tq is refused by the
 * launcher: LDPC_EHIP, and no kernel is started.
 */
int ldpc_debug_bp_decode_tq(const ldpc_graph *g, int tq, const float *d_llr, int B, int max_iters, float *d_post,
                            uint8_t *d_hard, int32_t *d_its, void *stream);

/*
 * Host-only: the launch plans of `count` ensemble soft-decoding calls on the (n, dv, dc)
 * shape (csrc/bp_plan.cpp bp_ens_plan).  calls[i] = {B, iters, algo, early_stop, mc,
 * want_post}; out[i] int64[9] = {path, threads, grid, LDS bytes, lds_slots, 0, slab bytes, -1,
 * scratch bytes}; names + 64 i: the kernel's display name, bp_ens_kernel<8|16|32,lds|gmem>.
 * One workgroup owns pad16(8 n dv + 4 n) bytes (messages, channel LLRs, cross index): in LDS
 * when that fits beside the early-stop syndrome bits and the Monte-Carlo curve, else one slab
 * of scratch per workgroup of the grid.  LDPC_EUNSUP when a call has no kernel (dc > 32).
 */
int ldpc_debug_ens_plan(int n, int dv, int dc, int count, const int32_t *calls, int cus, int64_t *out,
                        char *names);

/*
 * Host-only: the layer schedule of a CSR graph (csrc/graph_host.cpp build_layer_schedule): the
 * number of layers and layer[c] of every check c (layer: int32[m], may be NULL).  LDPC_EUNSUP
 * when the graph has none (an empty check, a check degree above 32, a check that holds a
 * variable twice).
 */
int ldpc_debug_layer_schedule(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                              const int32_t *var_slot, int n, int m, int32_t *num_layers, int32_t *layer);
/* The name of the rule ldpc_debug_layer_schedule colours by (a snapshot of a layered run records it). */
const char *ldpc_layer_rule(void);

/*
 * Host-only: the launch plans of `count` layered calls on one CSR graph (csrc/bp_plan.cpp
 * bp_layer_plan); calls / out / names as ldpc_debug_bp_plan, names
 * bp_layer_kernel<8|16|32,lds|gmem>.  LDPC_EUNSUP when the graph has no layer schedule.
 */
int ldpc_debug_layer_plan(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus,
                          int64_t *out, char *names);

/*
 * Host-only: the launch plans of `count` fixed-point layered calls on one CSR graph (csrc/bp_plan.cpp
 * bp_layer_q_plan); calls / out / names as ldpc_debug_layer_plan (algo is not read), names
 * bp_layer_q_kernel<8|16|32>, and column 4 of a row (lds_slots elsewhere) holds the number of
 * workgroups one CU holds at once.  A call whose block does not fit LDS gets the row of no plan
 * (name "none"): the decode entries return LDPC_EUNSUP for it.  LDPC_EUNSUP when the graph has no
 * layer schedule.
 */
int ldpc_debug_layer_q_plan(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                            const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus,
                            int64_t *out, char *names);
/* Host-only: LDPC_OK for a valid parameter set (the rules above), else LDPC_EINVAL. */
int ldpc_quant_check(const ldpc_quant *q);

/*
 * Host-only: the expansion of a quasi-cyclic code (ldpc_graph_create_qc's arguments and
 * convention) as the four CSR arrays of ldpc_graph_create_csr -- check_ptr int32[mb Z + 1],
 * check_var and var_slot int32[E] (E = Z x the number of non-zero cells), var_ptr
 * int32[nb Z + 1] -- and layer int32[mb Z], the block row of every check.  Any may be NULL.
 */
int ldpc_debug_qc_expand(int mb, int nb, int Z, const int32_t *base, int32_t *check_ptr, int32_t *check_var,
                         int32_t *var_ptr, int32_t *var_slot, int32_t *layer);
/*
 * Host-only: the launch plans of `count` fixed-point layered calls on a quasi-cyclic code; calls /
 * out / names as ldpc_debug_layer_q_plan, names bp_qc_q_kernel<64|256,8|16|32>: 64 threads (one
 * wave) when Z <= 64, else 256; the width by the largest block-row degree; the same LDS formula
 * and cap.  Under LDPC_NO_QC_KERNEL=1 the rows are bp_layer_q_kernel's on the block-row schedule.
 */
int ldpc_debug_qc_plan(int mb, int nb, int Z, const int32_t *base, int count, const int32_t *calls, int cus,
                       int64_t *out, char *names);
/*
 * Host-only: ldpc_debug_layer_q_plan and ldpc_debug_qc_plan in the codeword mode of
 * ldpc_mc_layered_q_cw_batch_dev.  The block gains, after the records, one bit per variable for
 * the codeword (4 ceil(n / 32) bytes); names, threads, grid and the cap are unchanged, and column 4
 * is recomputed from the new LDS.  has_desc != 0: a rate-matching description is given -- it adds
 * no LDS (the kernel re-reads the description for the count mask), so the rows are the same.  The
 * mode exists for Monte-Carlo calls only: a row with mc = 0 is the row of no plan.  LDPC_EUNSUP,
 * after every row is filled, when a row has no plan -- what ldpc_mc_layered_q_cw_batch_dev returns
 * for that call.
 */
int ldpc_debug_layer_q_cw_plan(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                               const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus,
                               int has_desc, int64_t *out, char *names);
int ldpc_debug_qc_cw_plan(int mb, int nb, int Z, const int32_t *base, int count, const int32_t *calls, int cus,
                          int has_desc, int64_t *out, char *names);

/*
 * Host-only: the launch plans of `count` BEC erasure-decoding calls on a graph of n variables
 * and m checks (csrc/bec_plan.cpp bec_plan); dc: the check degree of a regular graph, 0
 * otherwise (only the ensemble mode reads it).  calls[i] = {mode, B, iters, peel_cap}: mode 0
 * batch decode (words from memory), 1 fixed-code Monte-Carlo (fused channel), 2 ensemble
 * Monte-Carlo (graph per trial); peel_cap > 0 bounds the frontier lists as
 * ldpc_debug_peel_cap does.  out[i] int64[9] = {kernel, threads, W, plane bytes, codewords
 * per workgroup, grid, dynamic LDS bytes, F, LDS cap}: kernel 0 bec_kernel, 1
 * bec_dec_bits_kernel, 2 bec_mc_bits_kernel, 3 bec_peel_kernel, 4 none (the launch would
 * fail; the other columns are 0); W plane words per variable of plane bytes each (4: u32, 1:
 * u8; 0 for kernels 0 and 3); F the entries of each of bec_peel_kernel's frontier lists; LDS
 * cap the bound the LDS bytes were admitted under.  names + 64 i: the display name,
 * bec_kernel<T>, bec_dec_bits_kernel<T,W,u32|u8>, bec_mc_bits_kernel<T,W,u32|u8>,
 * bec_peel_kernel<1024> or none.
 */
int ldpc_debug_bec_plan(int n, int m, int dc, int count, const int32_t *calls, int64_t *out, char *names);

/*
 * Host-only: the launch plans of `count` Gallager A/B calls on a graph of n variables and E
 * slots (csrc/gb_plan.cpp gb_plan), from the shape alone.  calls[i] = {B, iters, early_stop, mc}:
 * mc 0 ldpc_gb_decode_batch_dev, 1 ldpc_mc_gb_batch_dev.  out[i] int64[8] = {threads, W, plane
 * bytes, codewords per workgroup, grid, dynamic LDS bytes, LDS cap, scratch bytes}: W plane
 * words per slot (1) of plane bytes each (4: u32, 2: u16, 1: u8); grid = ceil(B / codewords per
 * workgroup); scratch: the Monte-Carlo trial rows and iteration counts, 0 for a decode.  A call
 * whose planes fit LDS at no plane word (the entry returns LDPC_EUNSUP) is a row of zeros.
 * names + 64 i: the display name, gb_kernel<T,u32|u16|u8[,es][,mc]> or none.
 */
int ldpc_debug_gb_plan(int n, int E, int count, const int32_t *calls, int64_t *out, char *names);

/*
 * Host-only: the launch plan of one graph-sampler call (csrc/sample_plan.cpp sample_plan), from
 * the shape alone: n variables, m checks, E sockets, the largest check and variable degree,
 * regular != 0 for the (dv, dc) structure of ldpc_sample_regular (dv is read only then; pass
 * max_cdeg = dc, max_vdeg = dv), G graphs, and cus compute units (0: the single-pass form, no
 * search pass).  out int64[16] = {sequential (1) or one-level (0) sampler, threads of the draw
 * kernel, K buckets (0 for the sequential sampler), its dynamic LDS bytes, bw bitmap words,
 * bytes of a ring entry (2 | 4), fb counter bits (2 | 4 | 8, 0 from degree 256), fbu (fb when
 * the counters fit the bitmap's LDS), the emit pass's fb argument (-1: the variable-side kernel
 * follows), mdv = ceil(2^32 / dv) or 0 for the true divide (dv = 1, dv >= 256, irregular), V
 * variables per variable-side workgroup (0: no such kernel), nch chunks per graph, bytes of a
 * staged row entry (2 | 4), the variable-side kernel's dynamic LDS bytes, search workgroups
 * per CU, W persistent workgroups of the search pass (0: none)}; columns 4.. are 0 for the
 * one-level sampler.  names char[3][64]: the draw kernel (sample_seq_kernel<regular|csr,
 * u16|int>, sample_regular_kernel<256,u16,lds>, <512,u16,lds> or <1024,int32,gmem>), the
 * variable-side kernel (sample_var_side_kernel<1024,u16|int32> or none) and the search
 * kernel (sample_search_kernel<regular|csr,u16|int> or none).
 */
int ldpc_debug_sample_plan(int n, int m, int E, int max_cdeg, int max_vdeg, int regular, int dv, int G, int cus,
                           int64_t *out, char *names);

/*
 * Host-only: ldpc_mc_run's round accounting (csrc/mc_plan.hpp: per-slot batch clamp to
 * num_tests, the crossing slot's cut at its share of the remaining frame errors, later slots
 * dropped) driven by the same loop as the device run, on a synthetic trial sequence:
 * trial t is a frame error iff frame_error[t] != 0 (t < num_trials).  out int64[3] = {trials,
 * frame errors, rounds} -- equal to the sequential `while frame_errors < stop and trials <
 * num_tests` loop (parallel_simulator.py:198) for every ndev.  LDPC_EINVAL if the plan would
 * read past num_trials.
 */
int ldpc_debug_mc_plan(const uint8_t *frame_error, int64_t num_trials, int64_t num_tests, int64_t stop_frame_errors,
                       int batch, int ndev, int64_t *out);

/*
 * Host-only: which bp_loc_kernel instantiation family the local-edge layout of this CSR
 * graph (at T threads) would run on: 0 none (the graph takes another soft kernel), 1 the
 * (3,6) family <6,6,2,2> (every check degree 6, every variable degree 3), 2 the RSU family
 * <5,6,1,3> (check degrees 5..6, slot-0 variables degree 2, others 2..4).  Decided from the
 * whole layout shape, exactly as the device dispatch decides it.
 */
int ldpc_debug_loc_variant(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                           const int32_t *var_slot, int n, int m, int T, int32_t *variant);

/*
 * Device diagnostics: the sequential-draw sampler's counters accumulated since the last reset,
 * out uint64[32]: the search pass's 16 (attempts, aborted attempts, rounds, slots kept,
 * per-lane retry iterations, spread retry iterations, rounds with a repeated pick, help probes,
 * then s_memtime cycles: whole attempts, first draws, retries, marking, ring + validation,
 * compaction, claims; then failed validations), then the emit pass's 16.  Only a diagnostics build
 * (-DLDPC_SEQ_STATS=1) collects them; the product build returns LDPC_EUNSUP.
 */
int ldpc_debug_seq_stats(uint64_t *out, int reset);

/*
 * Device diagnostics of the ensemble BEC Monte-Carlo's frontier-peeling decoder
 * (csrc/peel.hip, the message_passing.c:7-82 semantics for the all-zero codeword), collected
 * by the product build on the current device since the last reset: out uint64[3] =
 * {iterations that ran the bitmap-snapshot scan because a frontier list overflowed, trials
 * with at least one such iteration, trials decoded}.  Evidence that the overflow branch ran
 * in a given launch.
 */
int ldpc_debug_peel_stats(uint64_t *out, int reset);

/*
 * Test-only: cap the peeling decoder's frontier-list capacity at F entries (F > 0) so the
 * overflow / scan branch runs deterministically at small n; F <= 0 restores the LDS budget's
 * capacity (5,266 entries at n = 64,800).  Process-wide; results stay bit-exact for any F.
 */
int ldpc_debug_peel_cap(int F);

/* Name of the soft kernel a graph dispatches to (tests / bench); early_stop: 0 fixed count,
 * 1 early stop with posteriors, 2 early stop with hard decisions only (d_post == NULL). */
const char *ldpc_bp_kernel_name(const ldpc_graph *g, int early_stop);

/* ---------------------------------------------------------------------- */
/* Misc                                                                    */
/* ---------------------------------------------------------------------- */
const char *ldpc_last_error(void);
int ldpc_device_count(void);
int ldpc_set_device(int device);
int ldpc_sync(void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_MI355X_H */
