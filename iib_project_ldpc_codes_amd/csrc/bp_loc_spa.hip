// bp_loc_kernel, sum-product instantiations, and bp_loc_chain_kernel (sum-product only).
#include "bp_loc.hpp"
#include "bp_loc_chain.hpp"

namespace ldpc {
hipError_t launch_loc_spa(const BpPlan &p, const ldpc_graph &g, BpArgs a, bool et, bool mc, hipStream_t s) {
    return launch_loc_algo<0>(p, g, a, et, mc, s);
}
}  // namespace ldpc
