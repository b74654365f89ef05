// The launch plan of a graph-sampler call: which draw kernel runs, its workgroup shape and LDS,
// the counter and row widths, the variable-side kernel and its chunks, the search pass and its
// grid.  Host-only and pure (no HIP call, no environment): sampler.hip launches what it says,
// tests/test_sample_plan.py reads it through ldpc_debug_sample_plan without a device.
#include "ldpc_internal.hpp"

namespace ldpc {
namespace {

constexpr int kWaveLanes = 64;
constexpr size_t kVarSideLds = 150 * 1024;  // the variable-side kernel's rows and counters

// One Rao-Sandelius level (sample_regular_kernel): the permutation as u16 in LDS where every
// variable id fits and the level has fewer than 1024 buckets, else as int32 in the caller's row
// on 1024 buckets.  LDS: cnt [K buckets][K / 64 waves] | wsum [16] | the u16 permutation.
void one_level(SamplePlan &p, int n, int E) {
    const int K = sample_buckets(E);
    const bool lds = n <= 65536 && K < 1024;
    // the instantiation: the shape table's row (kernel_shapes.hpp, what sampler.hip compiles).  Every
    // (buckets, lds) these rules give has one; a shape without a row would be no plan (threads = 0).
    const auto *row = shapes::find(shapes::kSampleLevel, [&](const shapes::SampleLevel &r) {
        return r.K == (lds ? K : 1024) && r.lds == lds;
    });
    if (!row) return;
    p.threads = p.K = row->K;
    p.lds = (size_t)4 * (p.K * (p.K / kWaveLanes) + 16) + (lds ? (size_t)2 * E : 0);
    p.draw = row->name;
}

}  // namespace

SamplePlan sample_plan(int n, int m, int E, int max_cdeg, int max_vdeg, bool regular, int dv, int G, int cus) {
    SamplePlan p;
    p.csr = !regular;
    p.seq = E >= kSeqMinE && E <= kSeqMaxE && max_cdeg <= kSeqMaxCdeg;
    if (!p.seq) {
        one_level(p, n, E);
        return p;
    }
    // bitmap words (a multiple of 4: cleared with 16-byte stores); rank counters of fb bits per
    // variable share them when they fit
    p.bw = ((E + 31) / 32 + 3) & ~3;
    p.fb = max_vdeg <= 3 ? 2 : (max_vdeg <= 15 ? 4 : (max_vdeg <= 255 ? 8 : 0));
    p.fbu = p.fb && (long)n * p.fb <= (long)p.bw * 32 ? p.fb : 0;
    p.ring = n <= 65536 ? 2 : 4;  // variable ids fit the u16 ring
    // the draw and search kernels' instantiation: the row of (csr, ring), as the launcher reads them.
    // Both choices have all four rows; a pair without one would be no plan (threads = 0).
    const auto *form = shapes::find(shapes::kSampleSeq, [&](const shapes::SampleSeq &r) {
        return r.csr == p.csr && r.ring == p.ring;
    });
    if (!form) return p;
    p.threads = kSeqThreads;
    p.lds = seq_plan_lds(p.bw, p.ring);
    p.draw = form->seq;
    p.mdv = regular && dv > 1 && dv < 256 ? (uint32_t)((0x100000000ull + dv - 1) / dv) : 0u;
    if (cus > 0 && G > 0) {
        // search pass: persistent workgroups, as many as fit the device (LDS bound), at most one
        // pool row each in the G rows of variable_lookup
        p.per_cu = (int)std::max<long>(1, std::min<long>(32, (long)kLdsMax / (long)p.lds));
        p.W = (int)std::min<long>((long)G, (long)cus * p.per_cu);
        p.search = form->search;
    }
    // variable side: chunks of V variables per workgroup after the emit pass, rows of at most
    // max_vdeg entries staged in LDS (u16 entries when every check / slot id fits) within 150 KiB
    const bool u16rows = regular ? m <= 65536 : E <= 65536;
    p.row = u16rows ? 2 : 4;
    if (p.fb) {
        const size_t bits = 8 * (size_t)p.row * (size_t)max_vdeg + (size_t)p.fb;  // LDS bits per variable
        p.V = (int)std::min<size_t>((size_t)n, kVarSideLds * 8 / bits) & ~63;
        if (p.V < 64) p.V = 0;
    }
    // the variable-side kernel's instantiation: the row of `row` (both widths have one; without
    // it there would be no such kernel, and the emit pass would do its work)
    const auto *vs = shapes::find(shapes::kSampleVarSide, [&](const shapes::SampleVarSide &r) { return r.row == p.row; });
    if (!vs) p.V = 0;
    p.emit_fb = p.V ? -1 : p.fbu;
    if (!p.V) return p;
    p.nch = (n + p.V - 1) / p.V;
    // counters (words, rounded up to 4) | rows
    p.vs_lds = (size_t)4 * ((((size_t)p.V * p.fb + 31) / 32 + 3) / 4 * 4) + (size_t)p.row * p.V * max_vdeg;
    p.var_side = vs->name;
    return p;
}

}  // namespace ldpc
