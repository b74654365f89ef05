// bp_ens_kernel: soft decoding over the random (dv, dc) ensemble -- codeword b on its own graph,
// rows b of the sampler's two lists -- and its launchers.
#include "kernel_args.hpp"

// ---------------------------------------------------------------------------
// 2c. Ensemble path: one workgroup decodes one codeword on the regular graph the sampler
//   (sampler.hip) wrote for it: check_lookup[b][E] (slot c*dc + j -> variable) and
//   variable_lookup[b][E] (edge v*dv + i -> check, ascending); cptr / vptr are implicit.  The
//   flooding loop of bp_flood.hpp in its ensemble view (variable sums from the channel LLR in
//   variable_lookup order) on those lists.
//   No host-built layout exists for such a graph, so the workgroup builds the one index the
//   lists lack -- the slot of every variable edge inside its check -- once per codeword, before
//   iteration 0: slot s of check c = s / dc holds variable v, and the edge of v that names c is
//   found by a scan of v's dv entries (unambiguous: the sampler rejects a repeated variable in a
//   check).  The index lives in the workgroup's own block, never in a [B][E] table.
//   Block: messages float[E] | channel LLRs float[n] | cross index int32[E] (ens_block_bytes).
//   The syndrome is kept as one bit per check in LDS (ens_syn_bytes: two buffers, filled and
//   read in alternate iterations): a variable decided 1 flips the bits of its dv checks
//   (slot / dc) with LDS atomics, so no per-slot decision byte is scattered to the slab.  Both
//   lists are only read.
// ---------------------------------------------------------------------------
#define LDPC_FLOOD_KERNEL bp_ens_kernel
#define LDPC_FLOOD_ARGS EnsArgs
#include "bp_flood.hpp"

namespace ldpc {
namespace {

EnsArgs ens_args(int n, int dv, int dc, const int32_t *chk, const int32_t *var, int B, int iters, float alpha) {
    EnsArgs a{};
    a.chk = chk;
    a.var = var;
    a.n = n;
    a.dv = dv;
    a.dc = dc;
    a.E = n * dv;
    a.m = a.E / dc;
    a.B = B;
    a.max_iters = iters;
    a.alpha = alpha;
    return a;
}

hipError_t launch_ens(EnsArgs a, float *d_scratch, size_t scratch_bytes, int algo, bool et, bool mc, hipStream_t s) {
    const BpPlan p = bp_ens_plan(a.n, a.dv, a.dc, a.B, a.max_iters, algo, et, mc, a.post != nullptr, device_cus());
    if (p.path == BpPath::None) return hipErrorNotSupported;
    // a caller that sized the buffer by another rule than bp_ens_plan's fails loudly
    if (p.scratch > (d_scratch ? scratch_bytes : 0)) return hipErrorInvalidValue;
    a.scratch = d_scratch;
    return launch_flood(p, a, algo, et, mc, s, BpPath::Ens8, hipErrorNotSupported);
}

}  // namespace

size_t ens_scratch_bytes(int n, int dv, int dc, int B, int iters, int algo, bool early_stop, bool mc, bool want_post) {
    return bp_ens_plan(n, dv, dc, B, iters, algo, early_stop, mc, want_post, device_cus()).scratch;
}

hipError_t launch_ens_decode(int n, int dv, int dc, const int32_t *check_lookup, const int32_t *variable_lookup,
                             const float *d_llr, int B, int max_iters, int algo, float alpha, int early_stop,
                             float *d_post, uint8_t *d_hard, int32_t *d_its, hipStream_t stream, float *d_scratch,
                             size_t scratch_bytes) {
    if (B <= 0) return hipSuccess;
    EnsArgs a = ens_args(n, dv, dc, check_lookup, variable_lookup, B, max_iters, alpha);
    a.llr = d_llr;
    a.post = d_post;
    a.hard = d_hard;
    a.its = d_its;
    return launch_ens(a, d_scratch, scratch_bytes, algo, early_stop != 0, false, stream);
}

hipError_t launch_mc_ens(int n, int dv, int dc, const int32_t *check_lookup, const int32_t *variable_lookup,
                         int channel, float p, float p2, uint64_t seed, uint64_t first_cw, int B, int max_iters,
                         int algo, float alpha, int early_stop, int32_t *trial, int32_t *trial_its,
                         hipStream_t stream, float *d_scratch, size_t scratch_bytes) {
    if (B <= 0) return hipSuccess;
    EnsArgs a = ens_args(n, dv, dc, check_lookup, variable_lookup, B, max_iters, alpha);
    a.ch = make_chan(channel, p, p2, seed);
    a.first_cw = first_cw;
    a.trial = trial;
    a.its = trial_its;
    return launch_ens(a, d_scratch, scratch_bytes, algo, early_stop != 0, true, stream);
}

}  // namespace ldpc
