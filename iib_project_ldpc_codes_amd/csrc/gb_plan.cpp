// The launch plan of a Gallager A/B call: gb_kernel's instantiation, its workgroup shape, grid and
// LDS.  Host-only and pure (no HIP call, no environment): gb.hip launches what it says,
// tests/test_gb_plan.py reads it through ldpc_debug_gb_plan without a device.
#include "ldpc_internal.hpp"

namespace ldpc {
namespace {

// gb_kernel's carve (gb.hip, M | Y | X | cnt | flag): one plane word per slot and per variable,
// the decision planes X only under early stop or Monte-Carlo, then one count per codeword of the
// workgroup and the three syndrome flags.
size_t gb_lds(int n, int E, bool has_x, int plane) {
    return pad16(((size_t)E + (has_x ? 2 : 1) * (size_t)n) * plane) + (size_t)4 * 8 * plane + 16;
}

}  // namespace

// The plane ladder: the widest plane word (u32, u16, u8) whose planes fit the cap -- a wider word
// decodes more codewords per instruction.  256 threads up to n = 2,048 (u32 planes always fit
// there: E <= 15 n), 1,024 beyond: such a workgroup fills most of a CU's LDS and is alone on it.
GbPlan gb_plan(int n, int E, int B, int iters, bool early_stop, bool mc) {
    GbPlan p;
    const bool has_x = early_stop || mc;
    for (int plane : {4, 2, 1}) {
        const size_t lds = gb_lds(n, E, has_x, plane);
        if (lds > kGbLdsCap) continue;
        // the instantiation: the shape table's row (kernel_shapes.hpp, what gb.hip compiles).  Every
        // (threads, plane) of this ladder has one; a shape without a row would be no plan.
        const int T = plane == 4 && n <= 2048 ? 256 : 1024;
        const auto *row = shapes::find(shapes::kGb, [&](const shapes::Gb &r) { return r.T == T && r.plane == plane; });
        if (!row) break;
        p.name = row->name[early_stop][mc];
        p.threads = T;
        p.W = 1;
        p.plane = plane;
        p.cw_per_wg = 8 * plane;
        p.grid = ((int64_t)B + p.cw_per_wg - 1) / p.cw_per_wg;
        p.lds = lds;
        p.cap = kGbLdsCap;
        p.scratch = mc ? (size_t)4 * B * ((size_t)iters + 2) : 0;
        break;
    }
    return p;
}

}  // namespace ldpc
