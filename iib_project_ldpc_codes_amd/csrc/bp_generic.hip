// bp_generic_kernel: any CSR graph with check degree <= 32, messages in LDS or in a
// per-workgroup global slab, and its launch ladder.
#include "kernel_args.hpp"

// 2b. Generic path: any (irregular) CSR graph, check degree <= MAXDC: the flooding loop of
//   bp_flood.hpp in its CSR view, on the host-built cptr / vptr / vslot.
#define LDPC_FLOOD_KERNEL bp_generic_kernel
#define LDPC_FLOOD_ARGS BpArgs
#include "bp_flood.hpp"

namespace ldpc {

hipError_t launch_generic(const BpPlan &p, const ldpc_graph &, BpArgs a, int algo, bool et, bool mc, hipStream_t s) {
    return launch_flood(p, a, algo, et, mc, s, BpPath::Generic8, hipErrorInvalidValue);
}

}  // namespace ldpc
