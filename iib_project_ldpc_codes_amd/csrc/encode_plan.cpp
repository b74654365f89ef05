// The launch plan of an encode call: encode_parity_kernel's tile width, its workgroup shape, grid
// and LDS, and the parity-plane scratch.  Host-only and pure (no HIP call, no environment):
// encode.hip launches what it says, tests/test_encode_plan.py reads it through
// ldpc_debug_encode_plan without a device.
#include "ldpc_internal.hpp"

namespace ldpc {

// The tile ladder: the widest tile (W = 4, 2, 1 plane words of 32 codewords) whose K information
// planes fit the cap -- a wider tile reads each word of A once for more codewords.
EncodePlan encode_plan(int n, int K, int rank, int B) {
    EncodePlan p;
    for (int W : {4, 2, 1}) {
        const size_t lds = (size_t)4 * K * W;
        if (lds > kEncLdsCap) continue;
        // the instantiation: the shape table's row (kernel_shapes.hpp, what encode.hip compiles).
        // Every W of this ladder has one; a tile without a row would be no plan.
        const auto *row = shapes::find(shapes::kEncTiles, [&](const shapes::EncTile &r) { return r.W == W; });
        if (!row) break;
        p.name = row->name;
        p.threads = lds > kLdsMax / 2 ? 1024 : 256;
        p.W = W;
        p.cw_per_wg = 32 * W;
        p.grid = ((int64_t)B + p.cw_per_wg - 1) / p.cw_per_wg;
        p.lds = lds;
        p.cap = kEncLdsCap;
        p.pwords = p.grid * W;
        p.scratch = (size_t)4 * p.pwords * rank;
        p.write_grid = ((int64_t)B * ((n + 3) / 4) + 255) / 256;
        break;
    }
    return p;
}

}  // namespace ldpc
