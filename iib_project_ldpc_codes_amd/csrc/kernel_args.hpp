// Kernel argument structs and the launch entries the kernel files give each other.
#pragma once
#include "device_common.hpp"
#include "ldpc_internal.hpp"

namespace ldpc {

struct BecArgs {
    const int32_t *cvar, *cptr, *vptr, *vchk;
    int n, m, dv, dc;  // dv, dc > 0: regular (pointers implicit)
    uint8_t *words;
    int32_t *errors, *its;
    int max_iters;
    // Monte-Carlo mode
    ChanArgs ch;
    uint64_t first_cw;
    int32_t *trial;  // [B][max_iters+1]
    // ensemble mode: codeword b decodes on its own graph (cvar / vchk + b*graph_stride)
    int64_t graph_stride;
};

struct BpArgs {
    const int32_t *cptr, *cvar, *vptr, *vslot;
    int n, m, E, B;
    const float *llr;
    float *post;
    uint8_t *hard;
    int32_t *its;
    int max_iters;
    float alpha;
    // Monte-Carlo mode
    ChanArgs ch;
    uint64_t first_cw;
    int32_t *trial;  // [B][max_iters+1]
    // generic kernel, messages in global scratch
    float *scratch;
    size_t scratch_bytes;  // (host) bytes at scratch: the plan's, a shorter buffer has been refused
    // LDS kernel lane layout (ldpc_graph::lane_var / lane_slot)
    const int32_t *lane_var, *lane_slot;
    int lds_slots;  // generic GMEM kernel: message slots [0, lds_slots) kept in LDS
    int wide_io;    // bp_loc_kernel / bp_loc_chain_kernel fixed count: 16-byte row I/O (BpPlan::wide_io); here, in what was padding: no other member moves
    // irregular kernel layout (ldpc_graph::irr_*)
    const int32_t *irr_lane, *irr_cdeg;
    int irr_KC, irr_S, irr_P;
    // local-edge kernel layout (ldpc_graph::loc_*)
    const int32_t *loc_var, *loc_pos, *loc_info;
    int loc_P, loc_ncls, loc_words;
    int loc_cls_q[5], loc_cls_d[4], loc_cls_w[5];
    uint32_t *work;  // bp_loc_kernel early stop (persistent grid): next-codeword counter (zeroed per launch); bp_loc_chain_kernel never reads it
};

// bp_ens_kernel: codeword b on graph b (rows b of the sampler's lists; cptr / vptr implicit)
struct EnsArgs {
    const int32_t *chk, *var;  // [B][E] slot c*dc + j -> variable; edge v*dv + i -> check, ascending
    int n, m, dv, dc, E, B;
    const float *llr;
    float *post;
    uint8_t *hard;
    int32_t *its;
    int max_iters;
    float alpha;
    // Monte-Carlo mode
    ChanArgs ch;
    uint64_t first_cw;
    int32_t *trial;  // [B][max_iters+1]
    float *scratch;  // <*,gmem>: one ens_block_bytes slab per workgroup
    int lds_slots;   // <*,gmem>: message slots [0, lds_slots) kept in LDS
};

// bp_layer_kernel: the layer schedule's tables (ldpc_graph::lay_*)
struct LayerArgs {
    const int32_t *tab, *var;
    int n, m, E, B, L;
    const float *llr;
    float *post;
    uint8_t *hard;
    int32_t *its;
    int max_iters;
    float alpha;
    // Monte-Carlo mode
    ChanArgs ch;
    uint64_t first_cw;
    int32_t *trial;  // [B][max_iters+1]
    float *scratch;  // <*,gmem>: one layer_block_bytes slab per workgroup
    int lds_slots;   // <*,gmem>: block words [0, lds_slots) kept in LDS
};

// bp_layer_q_kernel: the layer schedule's tables and the quantiser (ldpc_quant, validated)
struct LayerQArgs {
    const int32_t *tab, *var, *cbase;  // cbase [L]: the record of a layer's first check
    int n, m, B, L;
    const float *llr;
    int8_t *post;
    uint8_t *hard;
    int32_t *its;
    int max_iters;
    float scale;
    int Q, Pmax, norm8, offset;
    // Monte-Carlo mode
    ChanArgs ch;
    uint64_t first_cw;
    int32_t *trial;  // [B][max_iters+1]
};

// bp_qc_q_kernel: bp_layer_q_kernel's call and quantiser (q; its tab / var / cbase are not read, L
// is the number of block rows) and the quasi-cyclic code's row table (ldpc_graph::qc_row)
struct QcQArgs {
    LayerQArgs q;
    const int32_t *row;  // [L][kQcRow]: degree, then (column base, shift) per edge
    int Z;
};

// The codeword mode of the two fixed-point kernels (ldpc_mc_layered_q_cw_batch_dev): one more
// kernel argument behind the plain ones, which keep their layout
struct CwArgs {
    const uint32_t *desc;  // the rate-matching description, a dword per four positions; nullptr: all transmitted and counted
    const uint8_t *cw;     // [B][n] codewords, bit 0; nullptr: all-zero
    float known;           // |LLR| of a LDPC_RM_KNOWN position
    int vec;               // n % 4 == 0 and cw 4-byte aligned: the four codeword bytes of a group in one load
};

// gb_kernel (gb.hip): Gallager A/B on bit planes
struct GbArgs {
    const int32_t *cptr, *cvar, *vptr, *vslot;
    int n, m, E, dv, dc;  // dv, dc > 0: regular (pointers implicit)
    int B, max_iters, b;  // b: the flip threshold, 0 = Gallager A
    const uint8_t *bits;  // [B][n], bit 0 of each byte
    uint8_t *hard;        // [B][n] or nullptr
    int32_t *its;         // [B] or nullptr (Monte-Carlo: the trial iteration counts)
    // Monte-Carlo mode
    ChanArgs ch;
    uint64_t first_cw;
    int32_t *trial;  // [B][max_iters+1]
};

// The call's part of BpArgs, EnsArgs, LayerArgs or LayerQArgs (their field names agree; LayerQArgs
// has no alpha and int8 posteriors); the family's launch fills in its graph and layout.
template <typename Args>
Args call_args(const SoftCall &c) {
    Args a{};
    a.B = c.B;
    a.max_iters = c.max_iters;
    if constexpr (!std::is_same<Args, LayerQArgs>::value) a.alpha = c.alpha;
    a.llr = c.llr;
    a.post = static_cast<decltype(a.post)>(c.post);
    a.hard = c.hard;
    a.its = c.its;
    a.ch = c.ch;
    a.first_cw = c.first_cw;
    a.trial = c.trial;
    return a;
}

// One entry per soft kernel family (bp_lds.hip, bp_loc_spa.hip / bp_loc_ms.hip, bp_irr.hip,
// bp_generic.hip): launches the instantiation for (algo, early stop, Monte-Carlo) with the
// plan's grid, LDS and scratch layout.  The caller has checked the scratch buffer.
hipError_t launch_lds36(const BpPlan &p, const ldpc_graph &g, BpArgs a, int algo, bool et, bool mc, hipStream_t s);
hipError_t launch_loc_spa(const BpPlan &p, const ldpc_graph &g, BpArgs a, bool et, bool mc, hipStream_t s);
hipError_t launch_loc_ms(const BpPlan &p, const ldpc_graph &g, BpArgs a, bool et, bool mc, hipStream_t s);
hipError_t launch_irr(const BpPlan &p, const ldpc_graph &g, BpArgs a, int algo, bool et, bool mc, hipStream_t s);
hipError_t launch_generic(const BpPlan &p, const ldpc_graph &g, BpArgs a, int algo, bool et, bool mc, hipStream_t s);
// bp_layer_kernel (bp_layer.hip), from a bp_layer_plan
hipError_t launch_layer(const BpPlan &p, LayerArgs a, int algo, bool et, bool mc, hipStream_t s);
// bp_layer_q_kernel (bp_layer_q.hip), from a bp_layer_q_plan; cw: the codeword mode
// (the instantiation with a CwArgs, Monte-Carlo only), from a plan with its planes
hipError_t launch_layer_q(const BpPlan &p, const LayerQArgs &a, bool et, bool mc, const CwArgs *cw, hipStream_t s);
// bp_qc_q_kernel (bp_qc_q.hip), from a bp_layer_q_plan of a quasi-cyclic graph; cw as above
hipError_t launch_qc_q(const BpPlan &p, const QcQArgs &a, bool et, bool mc, const CwArgs *cw, hipStream_t s);
// Ensemble BEC Monte-Carlo by frontier peeling (peel.hip): launch_mc_bec_ensemble's BecKernel::Peel
// plans; trial b decodes on the (dv, dc) regular graph b of the two lists.
hipError_t launch_mc_bec_peel(const BecPlan &plan, int n, int m, int dv, int dc, const int32_t *check_lookup,
                              const int32_t *variable_lookup, float p, uint64_t seed, uint64_t first_cw, int max_iters,
                              int32_t *trial, int32_t *trial_its, hipStream_t stream);

namespace {
// Run-time (algo, early stop, Monte-Carlo) -> template arguments: f(int_c<ALGO>, bool_c<ET>, bool_c<MC>)
template <typename F>
hipError_t bp_modes(int algo, bool et, bool mc, F f) {
    auto with_mc = [&](auto A, auto E) { return mc ? f(A, E, bool_c<true>()) : f(A, E, bool_c<false>()); };
    auto with_et = [&](auto A) { return et ? with_mc(A, bool_c<true>()) : with_mc(A, bool_c<false>()); };
    return algo == 0 ? with_et(int_c<0>()) : with_et(int_c<1>());
}
}  // namespace

}  // namespace ldpc
