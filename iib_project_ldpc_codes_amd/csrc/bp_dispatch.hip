// Soft decoding: the exported launchers.  One bp_plan per call decides the kernel and its
// launch shape; the kernel families' own files (bp_lds.hip, bp_loc_*.hip, bp_irr.hip,
// bp_generic.hip) launch from it.
#include "kernel_args.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {
namespace {

BpArgs bp_args(const ldpc_graph &g, int B, int iters, float alpha) {
    BpArgs a{};
    a.cptr = g.cptr;
    a.cvar = g.cvar;
    a.vptr = g.vptr;
    a.vslot = g.vslot;
    a.n = g.n;
    a.m = g.m;
    a.E = g.E;
    a.B = B;
    a.max_iters = iters;
    a.alpha = alpha;
    return a;
}

hipError_t launch_bp(const ldpc_graph &g, BpArgs a, float *d_scratch, size_t scratch_bytes, int algo, bool et, bool mc,
                     hipStream_t s) {
    const BpPlan p = bp_plan(g, a.B, a.max_iters, algo, et, mc, a.post != nullptr, device_cus());
    // the one place a short buffer is refused: a caller that sized it by another rule than
    // bp_plan's fails loudly instead of writing past it
    if (p.scratch > (d_scratch ? scratch_bytes : 0)) return hipErrorInvalidValue;
    a.scratch = d_scratch;
    a.scratch_bytes = d_scratch ? scratch_bytes : 0;
    switch (p.path) {
        case BpPath::Loc: return algo == 0 ? launch_loc_spa(p, g, a, et, mc, s) : launch_loc_ms(p, g, a, et, mc, s);
        case BpPath::Lds36: return launch_lds36(p, g, a, algo, et, mc, s);
        case BpPath::Irr: return launch_irr(p, g, a, algo, et, mc, s);
        case BpPath::None: return hipErrorInvalidValue;
        default: return launch_generic(p, g, a, algo, et, mc, s);
    }
}

}  // namespace

int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    return cus;
}

size_t bp_scratch_bytes(const ldpc_graph &g, int B, int iters, int algo, bool early_stop, bool mc, bool want_post) {
    return bp_plan(g, B, iters, algo, early_stop, mc, want_post, device_cus()).scratch;
}

const char *bp_kernel_name(const ldpc_graph &g, int early_stop) {
    // early_stop 2: early stop, hard decisions only (no posteriors)
    return bp_plan(g, 1, 50, 0, early_stop != 0, false, early_stop != 2, device_cus()).name;
}

hipError_t launch_bp_decode(const ldpc_graph &g, const float *d_llr, int B, int max_iters, int algo,
                            float alpha, int early_stop, float *d_post, uint8_t *d_hard,
                            int32_t *d_its, hipStream_t stream, float *d_scratch, size_t scratch_bytes) {
    if (B <= 0) return hipSuccess;
    BpArgs a = bp_args(g, B, max_iters, alpha);
    a.llr = d_llr;
    a.post = d_post;
    a.hard = d_hard;
    a.its = d_its;
    return launch_bp(g, a, d_scratch, scratch_bytes, algo, early_stop != 0, false, stream);
}

hipError_t launch_mc_decode(const ldpc_graph &g, int channel, float p, float p2, uint64_t seed,
                            uint64_t first_cw, int B, int max_iters, int algo, float alpha, int early_stop,
                            int32_t *trial, int32_t *trial_its, hipStream_t stream, float *d_scratch,
                            size_t scratch_bytes) {
    if (B <= 0) return hipSuccess;
    if (channel == 0) return launch_mc_bec(g, p, p2, seed, first_cw, B, max_iters, trial, trial_its, stream);
    BpArgs a = bp_args(g, B, max_iters, alpha);
    a.ch = make_chan(channel, p, p2, seed);
    a.first_cw = first_cw;
    a.trial = trial;
    a.its = trial_its;
    return launch_bp(g, a, d_scratch, scratch_bytes, algo, early_stop != 0, true, stream);
}

// ---- the layered schedule: one bp_layer_plan per call, bp_layer.hip launches from it
namespace {

hipError_t launch_layered(const ldpc_graph &g, LayerArgs a, float *d_scratch, size_t scratch_bytes, int algo, bool et,
                          bool mc, hipStream_t s) {
    const BpPlan p = bp_layer_plan(g, a.B, a.max_iters, algo, et, mc, a.post != nullptr, device_cus());
    if (p.path == BpPath::None || !g.lay_tab || !g.lay_var) return hipErrorNotSupported;
    if (p.scratch > (d_scratch ? scratch_bytes : 0)) return hipErrorInvalidValue;  // as launch_bp
    a.tab = g.lay_tab;
    a.var = g.lay_var;
    a.n = g.n;
    a.m = g.m;
    a.E = g.E;
    a.L = g.lay_L;
    a.scratch = d_scratch;
    return launch_layer(p, a, algo, et, mc, s);
}

}  // namespace

size_t layer_scratch_bytes(const ldpc_graph &g, int B, int iters, int algo, bool early_stop, bool mc, bool want_post) {
    return bp_layer_plan(g, B, iters, algo, early_stop, mc, want_post, device_cus()).scratch;
}

hipError_t launch_layer_decode(const ldpc_graph &g, const float *d_llr, int B, int max_iters, int algo, float alpha,
                               int early_stop, float *d_post, uint8_t *d_hard, int32_t *d_its, hipStream_t stream,
                               float *d_scratch, size_t scratch_bytes) {
    if (B <= 0) return hipSuccess;
    LayerArgs a{};
    a.B = B;
    a.max_iters = max_iters;
    a.alpha = alpha;
    a.llr = d_llr;
    a.post = d_post;
    a.hard = d_hard;
    a.its = d_its;
    return launch_layered(g, a, d_scratch, scratch_bytes, algo, early_stop != 0, false, stream);
}

hipError_t launch_mc_layer(const ldpc_graph &g, int channel, float p, float p2, uint64_t seed, uint64_t first_cw,
                           int B, int max_iters, int algo, float alpha, int early_stop, int32_t *trial,
                           int32_t *trial_its, hipStream_t stream, float *d_scratch, size_t scratch_bytes) {
    if (B <= 0) return hipSuccess;
    LayerArgs a{};
    a.B = B;
    a.max_iters = max_iters;
    a.alpha = alpha;
    a.ch = make_chan(channel, p, p2, seed);
    a.first_cw = first_cw;
    a.trial = trial;
    a.its = trial_its;
    return launch_layered(g, a, d_scratch, scratch_bytes, algo, early_stop != 0, true, stream);
}

// ---- fixed-point layered min-sum: one bp_layer_q_plan per call, bp_layer_q.hip launches from it
namespace {

hipError_t launch_layered_q(const ldpc_graph &g, LayerQArgs a, const ldpc_quant &q, bool et, bool mc, hipStream_t s) {
    const BpPlan p = bp_layer_q_plan(g, a.B, a.max_iters, 1, et, mc, a.post != nullptr, device_cus());
    if (p.path == BpPath::None || !g.lay_tab || !g.lay_var || !g.lay_cbase) return hipErrorNotSupported;
    a.tab = g.lay_tab;
    a.var = g.lay_var;
    a.cbase = g.lay_cbase;
    a.n = g.n;
    a.m = g.m;
    a.L = g.lay_L;
    a.scale = q.scale;
    a.Q = (1 << (q.msg_bits - 1)) - 1;
    a.Pmax = (1 << (q.post_bits - 1)) - 1;
    a.norm8 = q.norm8;
    a.offset = q.offset;
    return launch_layer_q(p, a, et, mc, s);
}

}  // namespace

hipError_t launch_layer_q_decode(const ldpc_graph &g, const float *d_llr, int B, int max_iters, const ldpc_quant &q,
                                 int early_stop, int8_t *d_post, uint8_t *d_hard, int32_t *d_its, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    LayerQArgs a{};
    a.B = B;
    a.max_iters = max_iters;
    a.llr = d_llr;
    a.post = d_post;
    a.hard = d_hard;
    a.its = d_its;
    return launch_layered_q(g, a, q, early_stop != 0, false, stream);
}

hipError_t launch_mc_layer_q(const ldpc_graph &g, int channel, float p, float p2, uint64_t seed, uint64_t first_cw,
                             int B, int max_iters, const ldpc_quant &q, int early_stop, int32_t *trial,
                             int32_t *trial_its, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    LayerQArgs a{};
    a.B = B;
    a.max_iters = max_iters;
    a.ch = make_chan(channel, p, p2, seed);
    a.first_cw = first_cw;
    a.trial = trial;
    a.its = trial_its;
    return launch_layered_q(g, a, q, early_stop != 0, true, stream);
}

}  // namespace ldpc
