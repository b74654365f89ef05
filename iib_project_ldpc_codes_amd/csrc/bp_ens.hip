// bp_ens_kernel: soft decoding over the random (dv, dc) ensemble -- codeword b on its own graph,
// rows b of the sampler's two lists -- and its launch (EnsFamily, ldpc_internal.hpp).
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

hipError_t EnsFamily::launch(const BpPlan &p, const SoftCall &c, float *scratch, hipStream_t s) const {
    if (p.path == BpPath::None) return hipErrorNotSupported;
    EnsArgs a = call_args<EnsArgs>(c);
    a.chk = chk;
    a.var = var;
    a.n = n;
    a.dv = dv;
    a.dc = dc;
    a.E = n * dv;
    a.m = a.E / dc;
    a.scratch = scratch;
    return launch_flood(p, a, c.algo, c.early_stop, c.mc, s, BpPath::Ens8, hipErrorNotSupported);
}

}  // namespace ldpc
