// bp_loc_kernel, min-sum instantiations.
#include "bp_loc.hpp"

namespace ldpc {
hipError_t launch_loc_ms(const BpPlan &p, const ldpc_graph &g, BpArgs a, bool et, bool mc, hipStream_t s) {
    return launch_loc_algo<1>(p, g, a, et, mc, s);
}
}  // namespace ldpc
