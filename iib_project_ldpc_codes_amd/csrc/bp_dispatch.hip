// Soft decoding on a fixed code: the families' launches (ldpc_internal.hpp).  The caller's one
// plan per call says which kernel and its launch shape; the kernel families' own files
// (bp_lds.hip, bp_loc_*.hip, bp_irr.hip, bp_generic.hip, bp_layer.hip, bp_layer_q.hip, bp_qc_q.hip) launch from it.
#include "kernel_args.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {

int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    return cus;
}

const char *bp_kernel_name(const ldpc_graph &g, int early_stop) {
    // early_stop 2: early stop, hard decisions only (no posteriors)
    return bp_plan(g, 1, 50, 0, early_stop != 0, false, early_stop != 2, device_cus()).name;
}

hipError_t FloodFamily::launch(const BpPlan &p, const SoftCall &c, float *scratch, hipStream_t s) const {
    BpArgs a = call_args<BpArgs>(c);
    a.cptr = g.cptr;
    a.cvar = g.cvar;
    a.vptr = g.vptr;
    a.vslot = g.vslot;
    a.n = g.n;
    a.m = g.m;
    a.E = g.E;
    a.scratch = scratch;
    a.scratch_bytes = p.scratch;
    a.wide_io = p.wide_io;
    const bool et = c.early_stop, mc = c.mc;
    switch (p.path) {
        case BpPath::Loc: return c.algo == 0 ? launch_loc_spa(p, g, a, et, mc, s) : launch_loc_ms(p, g, a, et, mc, s);
        case BpPath::Lds36: return launch_lds36(p, g, a, c.algo, et, mc, s);
        case BpPath::Irr: return launch_irr(p, g, a, c.algo, et, mc, s);
        case BpPath::None: return hipErrorInvalidValue;
        default: return launch_generic(p, g, a, c.algo, et, mc, s);
    }
}

hipError_t LayerFamily::launch(const BpPlan &p, const SoftCall &c, float *scratch, hipStream_t s) const {
    if (p.path == BpPath::None || !g.lay_tab || !g.lay_var) return hipErrorNotSupported;
    LayerArgs a = call_args<LayerArgs>(c);
    a.tab = g.lay_tab;
    a.var = g.lay_var;
    a.n = g.n;
    a.m = g.m;
    a.E = g.E;
    a.L = g.lay_L;
    a.scratch = scratch;
    return launch_layer(p, a, c.algo, c.early_stop, c.mc, s);
}

hipError_t LayerQFamily::launch(const BpPlan &p, const SoftCall &c, float *, hipStream_t s) const {
    if (p.path == BpPath::None || !g.lay_tab || !g.lay_var || !g.lay_cbase) return hipErrorNotSupported;
    LayerQArgs a = call_args<LayerQArgs>(c);
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
    CwArgs cw{};
    if (c.cw_mode) {
        cw.desc = reinterpret_cast<const uint32_t *>(c.rm);
        cw.cw = c.cw;
        cw.known = c.known_llr;
        cw.vec = g.n % 4 == 0 && (reinterpret_cast<uintptr_t>(c.cw) & 3) == 0;
    }
    const CwArgs *cwp = c.cw_mode ? &cw : nullptr;
    if (p.path >= BpPath::QcQ64x8) {  // a quasi-cyclic graph on its row table
        if (!g.qc_row || g.qc_Z <= 0 || g.lay_L != g.qc_mb) return hipErrorNotSupported;
        a.L = g.qc_mb;
        return launch_qc_q(p, QcQArgs{a, g.qc_row, g.qc_Z}, c.early_stop, c.mc, cwp, s);
    }
    return launch_layer_q(p, a, c.early_stop, c.mc, cwp, s);
}

}  // namespace ldpc
