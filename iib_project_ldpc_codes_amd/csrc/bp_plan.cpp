// The launch plan of a soft-decoding call: which kernel runs, and its grid, LDS and scratch
// layout.  Host-only and pure (no HIP call): bp_dispatch.hip launches from it and answers the
// entry points' scratch-size and kernel-name questions from it, tests/test_bp_plan.py reads it
// through ldpc_debug_bp_plan without a device.
#include "ldpc_internal.hpp"

// Compile-time switches of the selection (scripts/build_variants.sh); LDPC_LDS36_PREFETCH and
// LDPC_GMEM_T, which the kernels' files read too, are in ldpc_internal.hpp.
#ifndef LDPC_LDS36_MINSUM
#define LDPC_LDS36_MINSUM 1  // (3,6) min-sum on bp_lds_kernel rather than bp_loc_kernel
#endif
#ifndef LDPC_LOC
#define LDPC_LOC 1  // fixed-count decode on bp_loc_kernel when the graph has a local-edge layout
#endif
#ifndef LDPC_LOC_CHAIN
#define LDPC_LOC_CHAIN 1  // fixed-count sum-product decodes on the chained layout where the graph has one
#endif
#ifndef LDPC_LOC_MSMC
#define LDPC_LOC_MSMC 1  // (3,6) min-sum Monte-Carlo (with or without early stop) on bp_loc_kernel
#endif
#ifndef LDPC_LOC_HARD_ET
#define LDPC_LOC_HARD_ET 1  // early-stop decodes without posteriors on bp_loc_kernel
#endif
#ifndef LDPC_LOC_ET_POST
#define LDPC_LOC_ET_POST 1  // early-stop decodes with posteriors on bp_loc_kernel (slab, persistent grid)
#endif
#ifndef LDPC_LOC_PERSIST
#define LDPC_LOC_PERSIST 1  // bp_loc_kernel early stop without posteriors: persistent grid on a counter (2: every launch; fixed count +0.4 %, noise)
#endif
#ifndef LDPC_LDS36_GRID
#define LDPC_LDS36_GRID 256  // persistent grid of the LDS kernel under early stop (one per CU)
#endif
#ifndef LDPC_GMEM_GRID
#define LDPC_GMEM_GRID 256  // one 1024-thread workgroup per CU, so the per-workgroup slabs stay cache-resident
#endif
#ifndef LDPC_GMEM_HYB
#define LDPC_GMEM_HYB 1  // first ~38k message slots in LDS, the rest in the slab
#endif

namespace ldpc {
namespace {

// messages | MC: per-iteration curve (16-byte padded) | min-sum MC: syndrome bits
size_t loc_lds_bytes(const GraphShape &g, int iters, bool mc, bool syn) {
    return pad16(loc_msg_words(g.loc_words, g.n) * 4) + (mc ? curve_bytes(iters) : 0) +
           (syn ? (size_t)((g.m + 31) / 32) * 4 : 0);
}
// Early stop with posteriors on bp_loc_kernel: a VP x T float2 slab per workgroup
size_t loc_ep_slab_bytes(const GraphShape &g) { return (size_t)(2 * g.loc_KP) * (size_t)g.loc_T * 2 * 4; }

// bp_irr_kernel: LDS bytes (messages, syndrome bits, curve) and whether the slab is used
size_t irr_lds_bytes(const GraphShape &g, int iters) {
    const int nsyn = (g.m + 31) >> 5;
    return pad16((size_t)g.irr_S * 4) + (size_t)((nsyn + 3) & ~3) * 4 + (size_t)(iters + 1) * 4;
}
bool irr_slab(const GraphShape &g) { return g.irr_S < g.irr_P; }

size_t lds36_bytes(const GraphShape &g, int iters, bool et, bool mc) {
    const size_t Ep = (size_t)lds_pair_span(g.m, 6) + kLdsDummy;
    size_t s = Ep * 4;
    if (et || mc) s = pad16(Ep * 5);
    if (mc) s += (size_t)(iters + 1) * 4;
    return s;
}

// bp_generic_kernel: every message (fp32) and sign byte of a codeword, and the posteriors
size_t generic_msg_bytes(const GraphShape &g) { return generic_block_bytes((size_t)g.n, (size_t)g.E); }
size_t generic_lds_bytes(const GraphShape &g, int iters, bool mc) {
    return generic_msg_bytes(g) + (mc ? (size_t)(iters + 1) * 4 : 0);
}

// bp_generic_kernel / bp_ens_kernel <*,gmem>: 1024-thread workgroups (the caller sets the grid
// and the slab of each); LDS holds `fixed` bytes (the curve, the syndrome bits) and
// the rest of the CU's LDS is filled with the first message slots.
void gmem_plan(BpPlan &p, size_t fixed, size_t E) {
    p.threads = LDPC_GMEM_T;
    const size_t room = fixed < kLdsMax - 4096 ? kLdsMax - 4096 - fixed : 0;
    p.lds_slots = LDPC_GMEM_HYB ? (int)std::min(E, room / 4) : 0;
    p.lds = fixed + (size_t)p.lds_slots * 4;
}

// The lane layout is present exactly when lane_T != 0 and the irregular one exactly when
// irr_VPT != 0: host_layouts (graph_host.cpp) sets each only next to a builder that returned
// non-empty arrays (build_lane_layout always fills T*VPT > 0 lanes; build_irr_layout's arrays are
// cleared when it refuses), and a graph whose upload failed is never handed out.
BpPath choose_path(const GraphShape &g, int iters, bool et, bool mc, int algo, bool hard_only) {
    if (!g.consistent) return BpPath::None;
    // min-sum on (3,6) codes with one 1024-thread local-edge workgroup per CU: bp_lds_kernel
    // is faster (its variable sums need no reordering); with the two-workgroup 512-thread
    // shape the local-edge kernel wins (bench code: 2.00 vs 1.74 M cw/s); the local-edge
    // kernel for everything else it covers
    // (Monte-Carlo with or without early stop; early-stop decodes with hard decisions only;
    // early-stop decodes that return posteriors when the message LDS can stage n posteriors +
    // n decision bytes (ep_ok: the persistent grid with per-workgroup slabs); min-sum early
    // stop: one check class)
    const bool lds36_ms = LDPC_LDS36_MINSUM && algo == 1 && g.lane_T && g.dv == 3 && g.dc == 6 && g.loc_T != 512;
    const bool one_cls = loc_variant(g) == kLocReg36;  // the one-class (3,6) instantiation
    // early stop with posteriors stages n posteriors + n decision bytes in the message LDS
    const bool ep_ok = LDPC_LOC_ET_POST && loc_msg_words(g.loc_words, g.n) * 4 >= (size_t)g.n * 5;
    const bool mode_ok = mc ? (algo == 0 || (LDPC_LOC_MSMC && one_cls))
                            : (!et || (LDPC_LOC_HARD_ET && (hard_only || ep_ok) && (algo == 0 || one_cls)));
    const bool mset = et && algo == 1;
    if (LDPC_LOC && mode_ok && iters > 0 && !lds36_ms && loc_variant(g) != kLocNone && loc_spare_ok(g.loc_words, g.n) &&
        loc_lds_bytes(g, iters, mc || mset, mset) <= kLdsMax - 2048)
        return BpPath::Loc;
    if (g.lane_T && g.dv == 3 && g.dc == 6 && lds36_bytes(g, iters, et, mc) <= kLdsMax - 2048)
        return BpPath::Lds36;
    if (g.irr_VPT && irr_lds_bytes(g, iters) <= kLdsMax - 1024) return BpPath::Irr;
    const int d = g.max_cdeg;
    if (d > 32) return BpPath::None;
    const bool lds = generic_lds_bytes(g, iters, mc) <= kLdsMax - 2048;
    if (d <= 8) return lds ? BpPath::Generic8 : BpPath::GenericG8;
    if (d <= 16) return lds ? BpPath::Generic16 : BpPath::GenericG16;
    return lds ? BpPath::Generic32 : BpPath::GenericG32;
}

}  // namespace

BpPlan bp_plan(const GraphShape &g, int B, int iters, int algo, bool et, bool mc, bool want_post, int cus) {
    algo = algo ? 1 : 0;
    BpPlan p;
    p.path = choose_path(g, iters, et, mc, algo, !want_post);
    p.grid = B;
    size_t slab_per_wg = 0;
    switch (p.path) {
        case BpPath::Loc: {
            p.name = "bp_loc_kernel";  // the family and its layout: bp_loc_kernel, or bp_loc_chain_kernel for p.chain
            p.threads = g.loc_T;
            const bool mset = et && algo == 1;
            p.lds = loc_lds_bytes(g, iters, mc || mset, mset);
            // fixed-count sum-product on a graph with a chained layout: its kernel (bp_loc_chain_kernel), its
            // tables and its (smaller) message LDS; every other mode keeps the plain layout
            p.chain = LDPC_LOC_CHAIN && g.chn_Tq > 0 && algo == 0 && !et && !mc && loc_spare_ok(g.chn_words, g.n);
            if (p.chain) p.lds = pad16(loc_msg_words(g.chn_words, g.n) * 4);
            // early stop with posteriors: persistent workgroups (two per CU, the most any
            // bp_loc_kernel shape keeps resident), each with a slab; early stop without: the same
            // grid on the counter alone
            const bool ep = et && !mc && want_post;
            p.persistent = ep || ((et || LDPC_LOC_PERSIST > 1) && LDPC_LOC_PERSIST);
            if (p.persistent) p.grid = std::min(B, 2 * cus);
            if (ep) slab_per_wg = loc_ep_slab_bytes(g);
            break;
        }
        case BpPath::Lds36:
            p.name = "bp_lds_kernel<3,6>";
            p.threads = g.lane_T;
            p.lds = lds36_bytes(g, iters, et, mc);
            // with early stop, one workgroup per CU striding over the codewords beats a
            // workgroup per codeword (+6 %: frames end at different iterations); fixed-count
            // decodes: +1 % with the prefetch
            if (et || (LDPC_LDS36_PREFETCH && !mc)) p.grid = std::min(B, LDPC_LDS36_GRID);
            break;
        case BpPath::Irr:
            p.name = irr_slab(g) ? "bp_irr_kernel<lds+slab>" : "bp_irr_kernel<lds>";
            p.threads = kIrrT;
            p.lds = irr_lds_bytes(g, iters);
            if (irr_slab(g)) {
                p.grid = std::min(B, LDPC_GMEM_GRID);
                slab_per_wg = (size_t)g.irr_P * 4;
            }
            break;
        case BpPath::Generic8:
        case BpPath::Generic16:
        case BpPath::Generic32:
            p.name = p.path == BpPath::Generic8    ? "bp_generic_kernel<8,lds>"
                     : p.path == BpPath::Generic16 ? "bp_generic_kernel<16,lds>"
                                                   : "bp_generic_kernel<32,lds>";
            p.threads = 256;
            p.lds = generic_lds_bytes(g, iters, mc);
            break;
        case BpPath::GenericG8:
        case BpPath::GenericG16:
        case BpPath::GenericG32: {
            p.name = p.path == BpPath::GenericG8    ? "bp_generic_kernel<8,gmem>"
                     : p.path == BpPath::GenericG16 ? "bp_generic_kernel<16,gmem>"
                                                    : "bp_generic_kernel<32,gmem>";
            p.grid = std::min(B, LDPC_GMEM_GRID);
            gmem_plan(p, mc ? curve_bytes(iters) : 0, (size_t)g.E);
            slab_per_wg = generic_msg_bytes(g);
            break;
        }
        default: return p;  // None (choose_path never gives an Ens* path: those are bp_ens_plan's)
    }
    p.width = p.chain ? g.chn_Tq : p.threads;
    // the chained call at a width that has an instantiation of its own
    if (p.chain && g.chn_tq)
        for (int tq : shapes::kLocChainTq)
            if (tq == g.chn_Tq) p.tq = tq;
    p.slab = slab_per_wg * (size_t)p.grid;
    p.scratch = p.slab;
    if (p.persistent) {
        p.counter = (long)p.slab;
        p.scratch += sizeof(uint32_t);
    }
    return p;
}

bool bp_wide_io(const BpPlan &p, const GraphShape &g, bool early_stop, bool mc, const void *llr, const void *post,
                const void *hard, bool narrow) {
    auto aligned = [](const void *q, uintptr_t to) { return (reinterpret_cast<uintptr_t>(q) & (to - 1)) == 0; };
    return p.path == BpPath::Loc && !early_stop && !mc && !narrow && g.n % 4 == 0 && aligned(llr, 16) &&
           aligned(post, 16) && aligned(hard, 4);
}

// bp_ens_kernel: the shape alone decides (every graph of the batch is (dv, dc) regular on n
// variables).  algo, early stop and want_post select the instantiation, not the layout.
BpPlan bp_ens_plan(int n, int dv, int dc, int B, int iters, int /*algo*/, bool /*early_stop*/, bool mc,
                   bool /*want_post*/, int cus) {
    BpPlan p;
    if (n <= 0 || dv <= 0 || dc <= 1 || dc > 32) return p;
    const size_t E = (size_t)n * (size_t)dv;
    const size_t block = ens_block_bytes((size_t)n, E), syn = ens_syn_bytes(E / (size_t)dc);
    const bool lds = block + syn + (mc ? (size_t)(iters + 1) * 4 : 0) <= kLdsMax - 2048;
    const int w = dc <= 8 ? 0 : (dc <= 16 ? 1 : 2);
    static const BpPath paths[2][3] = {{BpPath::EnsG8, BpPath::EnsG16, BpPath::EnsG32},
                                       {BpPath::Ens8, BpPath::Ens16, BpPath::Ens32}};
    static const char *const names[2][3] = {{"bp_ens_kernel<8,gmem>", "bp_ens_kernel<16,gmem>", "bp_ens_kernel<32,gmem>"},
                                            {"bp_ens_kernel<8,lds>", "bp_ens_kernel<16,lds>", "bp_ens_kernel<32,lds>"}};
    // one workgroup per CU striding over the batch: under early stop frames end at different
    // iterations, and the slabs of a gmem grid stay as few as the device can run at once
    p.grid = std::min(B, std::min(cus, LDPC_GMEM_GRID));
    size_t slab_per_wg = 0;
    if (lds) {
        p.threads = 256;
        p.lds = block + syn + (mc ? (size_t)(iters + 1) * 4 : 0);
    } else {
        const size_t fixed = (mc ? curve_bytes(iters) : 0) + syn;  // the curve, the syndrome bits
        if (fixed > kLdsMax - 4096) return BpPlan();               // no room for those alone: no kernel
        gmem_plan(p, fixed, E);
        slab_per_wg = block;
    }
    p.path = paths[lds][w];
    p.name = names[lds][w];
    p.slab = slab_per_wg * (size_t)p.grid;
    p.scratch = p.slab;
    return p;
}

// bp_layer_kernel: the graph's layer schedule and its size decide.  algo, early stop and
// want_post select the instantiation, not the layout.
BpPlan bp_layer_plan(const GraphShape &g, int B, int iters, int /*algo*/, bool /*early_stop*/, bool mc,
                     bool /*want_post*/, int cus) {
    BpPlan p;
    if (!g.consistent || g.lay_L <= 0 || g.max_cdeg > kLayerMaxD) return p;
    const size_t words = (size_t)g.n + (size_t)g.E, fixed = mc ? curve_bytes(iters) : 0;
    if (fixed > kLdsMax - 4096) return p;  // no room for the curve alone: no kernel
    const int w = g.max_cdeg <= 8 ? 0 : (g.max_cdeg <= 16 ? 1 : 2);
    static const BpPath paths[2][3] = {{BpPath::LayerG8, BpPath::LayerG16, BpPath::LayerG32},
                                       {BpPath::Layer8, BpPath::Layer16, BpPath::Layer32}};
    static const char *const names[2][3] = {
        {"bp_layer_kernel<8,gmem>", "bp_layer_kernel<16,gmem>", "bp_layer_kernel<32,gmem>"},
        {"bp_layer_kernel<8,lds>", "bp_layer_kernel<16,lds>", "bp_layer_kernel<32,lds>"}};
    // one budget for both forms (gmem_plan's): the block is wholly in LDS exactly when the slab
    // form would keep every word of it there
    const bool lds = fixed + words * 4 <= kLdsMax - 4096;
    size_t slab_per_wg = 0;
    if (lds) {
        p.threads = 256;
        p.grid = B;
        p.lds = fixed + words * 4;
    } else {
        // one workgroup per CU striding over the batch: the slabs stay as few as run at once
        p.grid = std::min(B, std::min(cus, LDPC_GMEM_GRID));
        gmem_plan(p, fixed, words);
        slab_per_wg = layer_block_bytes((size_t)g.n, (size_t)g.E);
    }
    p.path = paths[lds][w];
    p.name = names[lds][w];
    p.slab = slab_per_wg * (size_t)p.grid;
    p.scratch = p.slab;
    return p;
}

// bp_layer_q_kernel: the graph's layer schedule and its size decide; the block is in LDS or
// there is no kernel.  algo (min-sum only), early stop and want_post do not enter the layout.
BpPlan bp_layer_q_plan(const GraphShape &g, int B, int iters, int /*algo*/, bool /*early_stop*/, bool mc,
                       bool /*want_post*/, int /*cus*/) {
    return bp_layer_q_cw_plan(g, B, iters, mc, false);
}

BpPlan bp_layer_q_cw_plan(const GraphShape &g, int B, int iters, bool mc, bool cw) {
    BpPlan p;
    if (!g.consistent || g.lay_L <= 0 || g.max_cdeg > kLayerMaxD) return p;
    if (cw && !mc) return p;  // the codeword mode is a Monte-Carlo mode
    const size_t lds = (mc ? curve_bytes(iters) : 0) + (((size_t)g.n + 3) & ~(size_t)3) +
                       layer_q_record_bytes(g.max_cdeg) * (size_t)g.m + (cw ? layer_q_plane_bytes(g.n) : 0);
    if (lds > kLdsMax - 4096) return p;  // gmem_plan's budget; no slab form
    if (g.qc_Z > 0) {
        // a quasi-cyclic graph: bp_qc_q_kernel, one wave when a block row has no more checks
        // than that (three of a 256-thread workgroup's four waves would only wait at barriers)
        const int T = g.qc_Z <= 64 ? 64 : 256, D = g.max_cdeg <= 8 ? 8 : (g.max_cdeg <= 16 ? 16 : 32);
        const auto *r = shapes::find(shapes::kQcQ, [&](const shapes::QcQ &s) { return s.T == T && s.maxdc == D; });
        if (!r) return p;
        static_assert((int)BpPath::QcQ256x32 - (int)BpPath::QcQ64x8 + 1 == sizeof(shapes::kQcQ) / sizeof(shapes::kQcQ[0]),
                      "one BpPath per row of LDPC_QC_Q_SHAPES");
        p.path = static_cast<BpPath>((int)BpPath::QcQ64x8 + (int)(r - shapes::kQcQ));
        p.name = r->name;
        p.threads = T;
        p.grid = B;
        p.lds = lds;
        // informational: 32 wave slots of a CU, and kLdsMax bytes of LDS
        p.wg_per_cu = (int)std::min<size_t>(32 / (T / 64), kLdsMax / lds);
        return p;
    }
    const int w = g.max_cdeg <= 8 ? 0 : (g.max_cdeg <= 16 ? 1 : 2);
    static const BpPath paths[3] = {BpPath::LayerQ8, BpPath::LayerQ16, BpPath::LayerQ32};
    static const char *const names[3] = {"bp_layer_q_kernel<8>", "bp_layer_q_kernel<16>", "bp_layer_q_kernel<32>"};
    p.path = paths[w];
    p.name = names[w];
    p.threads = 256;
    p.grid = B;
    p.lds = lds;
    // a CU holds 32 waves (8 per SIMD) = eight 256-thread workgroups, and kLdsMax bytes of LDS
    p.wg_per_cu = (int)std::min<size_t>(8, kLdsMax / lds);
    return p;
}

}  // namespace ldpc
