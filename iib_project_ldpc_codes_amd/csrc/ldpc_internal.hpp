// Internal declarations shared by the host files (capi.cpp, mc_run.cpp, graph_host.cpp, graph_device.cpp, loc_layout.cpp,
// encode_host.cpp and the launch plans bp_plan.cpp, bec_plan.cpp, gb_plan.cpp, encode_plan.cpp, sample_plan.cpp) and the
// kernels (bec.hip, peel.hip, gb.hip, encode.hip, rate_match.hip, bp_*.hip, mc_kernels.hip, ml.hip, sampler.hip).  Not part of the public
// ABI (see include/ldpc_mi355x.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "kernel_shapes.hpp"

struct ldpc_quant;  // include/ldpc_mi355x.h

// Shape of a prepared Tanner graph: every scalar of the graph and of its kernel layouts, filled
// on the host (host_layouts, graph_host.cpp).  All that the launch plan (bp_plan.cpp) and the
// launchers' sizing read; no device is involved.  Slot e = position in the check-major edge
// list (the reference's check_lookup order, random_code_generator.c:34-36).
struct GraphShape {
    int n = 0, m = 0, k = 0, E = 0;
    int dv = 0, dc = 0;          // > 0 when every variable / check has that degree
    int max_vdeg = 0, max_cdeg = 0;
    bool consistent = false;     // vslot defined: soft decoding allowed
    int vchk_len = 0;            // length of vchk (E')
    // Conflict-aware lane layout of the LDS-resident (3,6) kernel (build_lane_layout,
    // graph_host.cpp): position p = t + i*T is thread t's i-th variable; every 32 consecutive
    // positions form one half-wave LDS access.  lane_T == 0: none.
    int lane_T = 0, lane_VPT = 0;
    // Layout of the irregular kernel (bp_irr_kernel; build_irr_layout, graph_host.cpp):
    // check c = k*1024 + t (thread t, row k < irr_KC), its slot j at position
    // (k*irr_DC + j)*1024 + t; positions [0, irr_S) live in LDS, [irr_S, irr_P) in a
    // per-workgroup global slab.  Lane p = i*1024 + t is thread t's i-th variable.  irr_VPT == 0: none.
    int irr_VPT = 0, irr_KC = 0, irr_DC = 0, irr_S = 0, irr_P = 0;
    // Local-edge layout of bp_loc_kernel (build_loc_layout, loc_layout.cpp); loc_KP == 0: none
    int loc_T = 0, loc_KP = 0, loc_DVN = 0, loc_P = 0, loc_ncls = 0, loc_words = 0, loc_dlo = 0, loc_dhi = 0;
    int loc_dvn0 = 0, loc_dvn1 = 0;       // non-local edges per variable, local slot 0 / 1 (max)
    bool loc_abs0 = false, loc_abs1 = false;  // some variable of that slot has fewer
    int loc_cls_q[5] = {0}, loc_cls_d[4] = {0}, loc_cls_w[5] = {0};
    // Chained local-edge layout beside it (build_loc_chain_layout; fixed-count sum-product
    // decodes run on it); chn_Tq == 0: none
    int chn_Tq = 0, chn_words = 0;
    // ... on the instantiation with that Tq as a constant where kernel_shapes.hpp lists one (false:
    // LDPC_NO_LOC_TQ=1, the generic instantiation at every width)
    bool chn_tq = true;
    // Layer schedule of bp_layer_kernel (build_layer_schedule, graph_host.cpp): lay_L layers, the
    // largest of lay_max checks; lay_L == 0: none
    int lay_L = 0, lay_max = 0;
    // Quasi-cyclic graph (host_graph_from_qc): its layers are its block rows (kQcLayerRule), not a
    // colouring; qc_Z > 0: the mb x nb array of Z x Z blocks behind it, for bp_qc_q_kernel's
    // row table (qc_row).  0 for every other graph, and for a quasi-cyclic one kept on the table kernels.
    bool lay_block_rows = false;
    int qc_Z = 0, qc_mb = 0, qc_nb = 0;
};

// Device-resident Tanner graph: the shape and the device arrays (listed once more, each with the
// host vector it is filled from, in graph_device.cpp's for_graph_arrays).
struct ldpc_graph : GraphShape {
    int device = 0;
    int32_t *cvar = nullptr;     // [E]   variable of each slot (check-major)
    int32_t *cptr = nullptr;     // [m+1] check c owns slots [cptr[c], cptr[c+1])
    int32_t *vptr = nullptr;     // [n+1] variable v owns edges [vptr[v], vptr[v+1])
    int32_t *vchk = nullptr;     // [E']  BEC: check id of each variable edge, -1 when
                                 //       that check holds v != 1 times (never assigns)
    int32_t *vslot = nullptr;    // [E]   soft: slot of each variable edge (consistent only)
    int32_t *lane_var = nullptr;   // [T*VPT]    variable id, -1 = padding lane
    int32_t *lane_slot = nullptr;  // [T*VPT*dv] LDS position per edge (lds_pair_pos; padding
                                   //            lanes: dummy positions >= lds_pair_span)
    int32_t *irr_lane = nullptr;  // [3][1024*VPT]: variable id (-1 pad), positions j0|j1<<16, j2|j3<<16
                                  // (0xFFFF = no edge; lanes of one 64-lane row share a degree)
    int32_t *irr_cdeg = nullptr;  // [2][1024]: degrees of thread t's checks, 4 bits per row k
    int32_t *loc_var = nullptr;   // [2*KP][2][T] variable id of var pair (thread, pair slot) half h, -1 pad
    int32_t *loc_pos = nullptr;   // [2*KP][DVN][T] non-local edge u's LDS words, h=0 | h=1 << 16
    int32_t *loc_info = nullptr;  // [2*KP][T] bit u + 4h: edge u present; bits 8+2h: local edge index jl;
                                  // bit 16 + 4h + jl: the same one-hot (min-sum order masks)
    int32_t *chn_var = nullptr, *chn_pos = nullptr, *chn_info = nullptr;  // the chained layout's, same formats
    // layer schedule (LayerSchedule, graph_host.hpp): lay_tab [L][kLayerTab] per-layer offsets,
    // lay_var [E] variables, layer-ordered and lane-major
    int32_t *lay_tab = nullptr, *lay_var = nullptr;
    int32_t *lay_cbase = nullptr;  // [L+1] checks before each layer (LayerSchedule::ptr): bp_layer_q_kernel's record base
    int32_t *qc_row = nullptr;     // [qc_mb][kQcRow] degree and (column base, shift) pairs of each block row (qc_Z > 0)
};

// Local-edge layout (loc_layout.cpp): see the comment there.
constexpr int kLocMaxD = 8, kLocMaxCls = 4;
struct LocLayout {
    int T = 1024, KP = 0, DVN = 0, P = 0, ncls = 0, words = 0;
    int DVN0 = 0, DVN1 = 0;     // non-local edges per variable of local slot 0 / 1 (max)
    bool ABS0 = false, ABS1 = false;  // some variable of that slot has fewer
    long conflicts = 0;  // sum over (instruction, half wave) of the busiest bank's extra lanes
    int cls_q[kLocMaxCls + 1] = {0}, cls_d[kLocMaxCls] = {0}, cls_w[kLocMaxCls + 1] = {0};
    std::vector<int32_t> var, pos, info;
};
bool build_loc_layout(int n, int m, const std::vector<int32_t> &cptr, const std::vector<int32_t> &cvar,
                      const std::vector<int32_t> &vptr, const std::vector<int32_t> &vslot, LocLayout &L);

// Chained local-edge layout (loc_layout.cpp, "Chained layout"): the (3,6) T = 512, KP = 5 shape
// with the five .x (and the five .y) checks of a thread on a path whose links are the checks'
// slot-1 local variables, so the edge from each link variable to the next check of the path stays
// in a VGPR too.  Built beside the plain layout; Tq == 0: none.
constexpr int kLocChainT = 512, kLocChainKP = 5, kLocChainCL = kLocChainKP - 1;
struct LocChainLayout {
    int Tq = 0;          // threads that own check pairs: pair q = t + k Tq (t < Tq, k < KP)
    int words = 0;       // LDS message words (32 Tq)
    long conflicts = 0;  // as LocLayout::conflicts
    // var, pos, info: LocLayout's formats at T = 512 (var pairs 2k + 1, k < KP - 1: one LDS edge,
    // row 0 of pos); chk[(2k + h) T + t]: the check at pair slot k, half h of thread t (-1: none)
    std::vector<int32_t> var, pos, info, chk;
};
bool build_loc_chain_layout(int n, int m, const std::vector<int32_t> &cptr, const std::vector<int32_t> &cvar,
                            const std::vector<int32_t> &vptr, const std::vector<int32_t> &vslot, const LocLayout &plain,
                            LocChainLayout &C);

// Check-degree range of a layout's classes (a mixed class counts its smaller check); false
// when a mixed class is not (dhi - 1, dhi) -- the kernel pads a mixed pair's smaller check by
// exactly one input.
inline bool loc_degree_range(const LocLayout &L, int &dlo, int &dhi) {
    dlo = 99;
    dhi = 0;
    for (int i = 0; i < L.ncls; ++i) {
        dlo = std::min(dlo, L.cls_d[i] >> 8 ? L.cls_d[i] >> 8 : L.cls_d[i]);
        dhi = std::max(dhi, L.cls_d[i] & 255);
    }
    bool ok = true;
    for (int i = 0; i < L.ncls; ++i)
        if (L.cls_d[i] >> 8) ok &= (L.cls_d[i] & 255) == dhi && (L.cls_d[i] >> 8) == dhi - 1;
    return ok;
}

// The local-edge scalars of a graph's shape, from its built layout; loc_KP = 0 (no layout the
// kernel can run) when the degree mix is outside loc_degree_range.
inline void loc_shape(const LocLayout &K, GraphShape &g) {
    g.loc_T = K.T; g.loc_KP = K.KP; g.loc_DVN = K.DVN; g.loc_P = K.P;
    g.loc_ncls = K.ncls; g.loc_words = K.words;
    if (!loc_degree_range(K, g.loc_dlo, g.loc_dhi)) g.loc_KP = 0;
    for (int i = 0; i <= K.ncls; ++i) { g.loc_cls_q[i] = K.cls_q[i]; g.loc_cls_w[i] = K.cls_w[i]; }
    for (int i = 0; i < K.ncls; ++i) g.loc_cls_d[i] = K.cls_d[i];
    g.loc_dvn0 = K.DVN0; g.loc_dvn1 = K.DVN1;
    g.loc_abs0 = K.ABS0; g.loc_abs1 = K.ABS1;
}

// The bp_loc_kernel instantiation family a local-edge layout runs on -- decided from the
// WHOLE shape, never from the check degrees alone (a check-regular degree-6 graph with
// variable degrees {2, 4} has loc_dlo == 6 but needs the RSU family's DVN = 3 rows):
//   kLocReg36: <DLO=6, DHI=6, DVN0=2, DVN1=2, ABS0=ABS1=false> -- every check degree 6 and every
//              variable degree 3 (the (3,6) codes)
//   kLocRsu:   <DLO=5, DHI=6, DVN0=1, DVN1=3, ABS0=false, ABS1=true> -- check degrees 5..6, every
//              slot-0 variable degree 2, slot-1 variables degree 2..4
//   kLocNone:  no instantiation (the graph runs on bp_lds / bp_irr / bp_generic)
// Each family has the (T, KP) rows of its shape table (kernel_shapes.hpp), which bp_loc.hpp instantiates; the chained layout's kernel (bp_loc_chain.hpp) has the one shape kLocChainT x kLocChainKP.
enum LocVariant { kLocNone = 0, kLocReg36 = 1, kLocRsu = 2 };
inline int loc_variant(int dlo, int dhi, int DVN, int dvn0, int dvn1, bool abs0, bool abs1, int T, int KP) {
    if (KP <= 0) return kLocNone;
    const bool reg36 = dlo == 6 && dhi == 6 && DVN == 2 && dvn0 == 2 && dvn1 == 2 && !abs0 && !abs1;
    const bool rsu = !reg36 && dlo >= 5 && dhi == 6 && DVN == 3 && dvn0 == 1 && !abs0 && dvn1 <= 3;
    const auto row = [&](const ldpc::shapes::Shape2 &r) { return r.T == T && r.per_thread == KP; };
    if (reg36 && ldpc::shapes::find(ldpc::shapes::kLocReg36, row)) return kLocReg36;
    if (rsu && ldpc::shapes::find(ldpc::shapes::kLocRsu, row)) return kLocRsu;
    return kLocNone;
}
inline int loc_variant(const GraphShape &g) {
    return loc_variant(g.loc_dlo, g.loc_dhi, g.loc_DVN, g.loc_dvn0, g.loc_dvn1, g.loc_abs0, g.loc_abs1, g.loc_T, g.loc_KP);
}

// Irregular kernel (bp_irr_kernel): 1024 threads; LDS room for messages (bytes)
// after the early-stop syndrome bits and the Monte-Carlo curve.
constexpr int kIrrT = 1024;
constexpr size_t kIrrLdsMsgBytes = 148 * 1024;

// Threads per workgroup and variables per thread of the LDS-resident kernel
// for block length n: >= 2 % spare lanes for the conflict-aware layout.  (At
// n = 10^4, 3 % spare = 11 variables per thread packs with ~1.02 LDS cycles per
// half-wave access, 2 % = 10 per thread with ~1.5 -- and is 5 % faster: the
// variable phase is bound by per-lane work, not bank conflicts.)  The first row of the shape
// table (kernel_shapes.hpp, what bp_lds.hip instantiates) with enough lanes: the 256-thread rows
// up to n = 2048, the 1024-thread rows beyond and where those do not reach.
#ifndef LDPC_LDS_SPARE
#define LDPC_LDS_SPARE 102  // lanes >= n * SPARE / 100 (fewer lanes beat fewer bank conflicts)
#endif
inline bool lds_shape(int n, int &T, int &VPT) {
    const long need = ((long)n * LDPC_LDS_SPARE + 99) / 100;
    for (int t : {256, 1024}) {
        if (t == 256 && n > 2048) continue;
        T = t;
        const auto *r = ldpc::shapes::find(ldpc::shapes::kLds36, [&](const ldpc::shapes::Shape2 &s) {
            return s.T == t && (long)t * s.per_thread >= need;
        });
        if (r) { VPT = r->per_thread; return true; }
    }
    return false;
}
constexpr size_t kLdsMax = 160 * 1024;  // LDS bytes of one CU (the launch plans budget against it)
// Dynamic-LDS caps of the BEC kernels (bec_plan.cpp): bec_kernel and bec_peel_kernel keep static
// LDS (block_sum's partial sums, the list control words) beside the dynamic part; a bit-sliced
// workgroup may fill the CU, and takes more than one word per variable only while two
// workgroups still fit a CU.
constexpr size_t kBecWordLdsCap = kLdsMax - 1024, kPeelLdsCap = kLdsMax - 1024;
constexpr size_t kBecBitsLdsCap = kLdsMax - 4096, kBecBitsWideLdsCap = 72 * 1024;
constexpr int kLdsDummy = 3 * 32 + 4;  // dummy message slots after the real ones (DV=3)

// Message positions of the LDS-resident (3,6) kernel.  Checks are paired
// (2q, 2q+1) and their edges interleaved, [pair q][edge][check of the pair], so
// one LDS access moves the same edges of both checks and the check update runs
// on float2 (both checks in every packed VALU op).  With a 2*dc = 12-dword pair
// stride the check phase's ds_read_b128 / ds_write_b128 are conflict-free.
inline int lds_pair_pos(int slot, int dc) {
    const int c = slot / dc, j = slot % dc;
    return (c >> 1) * 2 * dc + 2 * j + (c & 1);
}
// Positions spanned by the m checks (an odd m leaves one phantom check).
inline int lds_pair_span(int m, int dc) { return ((m + 1) / 2) * 2 * dc; }

namespace ldpc {

void set_error(const std::string &msg);
constexpr size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }  // LDS carves keep 16-byte alignment
// bp_loc_kernel's message LDS in words: the layout's message words and its 64 dummy words, or the
// n staged channel values / posteriors, whichever is more.  The plan takes the kernel only for a
// layout that leaves kLocSpare spare words behind the n staged values (loc_spare_ok; every layout
// the builders make does: a variable has a non-local edge): the fixed-count decodes' unguarded row
// I/O sends what lies past variable n - 1 there.
constexpr int kLocSpare = 4;
constexpr size_t loc_msg_words(int words, int n) { return (size_t)(words + 64 > n ? words + 64 : n); }
constexpr bool loc_spare_ok(int words, int n) { return words + 64 >= n + kLocSpare; }

// The launch plan of one BEC call (bec_plan.cpp): which kernel runs and everything its launch
// needs, decided in one host-only function; bec.hip and peel.hip launch what it says.
enum class BecMode { Decode, Mc, EnsMc };  // words from memory | fixed code, fused channel | graph per trial
enum class BecKernel { Word, DecBits, McBits, Peel, None };
struct BecPlan {
    BecKernel kernel = BecKernel::None;
    const char *name = "none";  // display name, e.g. bec_dec_bits_kernel<256,2,u32>
    int threads = 0;
    int W = 0, plane = 0;    // bit-sliced: plane words per variable and bytes of one (4: u32, 1: u8)
    int cw_per_wg = 0;       // codewords of one workgroup (1: bec_kernel, bec_peel_kernel)
    int64_t grid = 0;
    size_t lds = 0;          // dynamic LDS bytes
    size_t cap = 0;          // the cap `lds` was admitted under (one of the four above)
    int F = 0;               // bec_peel_kernel: entries of each frontier list
};
// dc: the check degree of a regular graph (read under EnsMc); peel_cap > 0: a test's bound on F (peel_cap()).
BecPlan bec_plan(int n, int m, int dc, int B, int iters, BecMode mode, int peel_cap);

// The launch plan of one Gallager A/B call (gb_plan.cpp): gb_kernel's instantiation, grid and LDS,
// decided in one host-only function; gb.hip launches what it says.  One workgroup decodes one plane
// word of codewords (8 * plane of them); threads == 0: the planes fit LDS at no plane word.
constexpr size_t kGbLdsCap = kLdsMax - 4096;
constexpr int kGbMaxVdeg = 15, kGbMaxB = 14;  // four count planes
struct GbPlan {
    const char *name = "none";  // display name, e.g. gb_kernel<1024,u16,es,mc>
    int threads = 0;
    int W = 0, plane = 0;    // plane words per slot (1) and bytes of one (4: u32, 2: u16, 1: u8)
    int cw_per_wg = 0;
    int64_t grid = 0;
    size_t lds = 0;          // dynamic LDS bytes
    size_t cap = 0;          // the cap `lds` was admitted under (kGbLdsCap)
    size_t scratch = 0;      // Monte-Carlo: bytes of the trial rows and iteration counts; else 0
};
GbPlan gb_plan(int n, int E, int B, int iters, bool early_stop, bool mc);

// Kernel launchers (bec.hip, bp_dispatch.hip, bp_ens.hip, mc_kernels.hip, ml.hip).  All asynchronous on `stream`.
// Return hipSuccess or the launch error.
hipError_t launch_bec_decode(const ldpc_graph &g, uint8_t *d_words, int B, int max_iters,
                             int32_t *d_errors, int32_t *d_its, hipStream_t stream);

// Compile-time switches read on both sides of the launch (the rest: bp_plan.cpp, the kernels' files)
#ifndef LDPC_LDS36_PREFETCH
#define LDPC_LDS36_PREFETCH 1  // persistent LDS kernel (decode API) prefetching the next codeword's LLRs
#endif
#ifndef LDPC_GMEM_T
#define LDPC_GMEM_T 1024  // threads of bp_generic_kernel<*,gmem>: one workgroup per CU
#endif

// The launch plan of one soft-decoding call (bp_plan.cpp): which kernel runs and everything the
// launch needs, decided in one host-only function, once per call.  The scratch request, the
// families' launches and the kernel-name introspection all read it; nothing else re-derives these numbers.
enum class BpPath {
    Loc, Lds36, Irr, Generic8, Generic16, Generic32, GenericG8, GenericG16, GenericG32, None,
    // bp_ens_kernel (bp_ens_plan only; listed after None so the values above stay as they were)
    Ens8, Ens16, Ens32, EnsG8, EnsG16, EnsG32,
    // bp_layer_kernel (bp_layer_plan only)
    Layer8, Layer16, Layer32, LayerG8, LayerG16, LayerG32,
    // bp_layer_q_kernel (bp_layer_q_plan only)
    LayerQ8, LayerQ16, LayerQ32,
    // bp_qc_q_kernel<T,MAXDC> (bp_layer_q_plan on a quasi-cyclic graph), in the order of LDPC_QC_Q_SHAPES
    QcQ64x8, QcQ64x16, QcQ64x32, QcQ256x8, QcQ256x16, QcQ256x32
};
struct BpPlan {
    BpPath path = BpPath::None;
    const char *name = "none";  // display name (ldpc_bp_kernel_name)
    int threads = 0, grid = 0;
    // bp_plan: the threads a workgroup is launched with -- the chained layout's Tq (only its threads
    // t < Tq own anything; `threads` stays its instantiation's T, the stride of its tables), else `threads`
    int width = 0;
    // bp_plan: the chained call's compile-time width -- `width` when LDPC_LOC_CHAIN_TQ (kernel_shapes.hpp) lists it,
    // the instantiation bp_loc_chain_kernel<KP, T, tq>; 0: the generic instantiation, and every other call
    int tq = 0;
    size_t lds = 0;            // dynamic LDS bytes
    int lds_slots = 0;          // bp_generic_kernel / bp_ens_kernel <*,gmem>: message slots [0, lds_slots) kept in LDS
    bool chain = false;         // the chained layout's kernel (bp_loc_chain_kernel) and tables; the plan's name stays the family's
    bool wide_io = false;       // bp_loc_kernel / bp_loc_chain_kernel, fixed count: 16-byte row I/O (bp_wide_io; FloodFamily::plan sets it)
    bool persistent = false;    // bp_loc_kernel: the grid pulls codewords from a counter in scratch
    size_t slab = 0;            // bytes of per-workgroup slabs at the start of scratch (0: none)
    long counter = -1;          // byte offset of the work counter in scratch (-1: none)
    size_t scratch = 0;         // total scratch bytes the launch needs
    int wg_per_cu = 0;          // bp_layer_q_kernel: workgroups a CU holds at once (LDS and wave slots)
};
// cus: compute units of the device (device_cus()); mc: fused-channel Monte-Carlo; want_post: a
// decode that returns posteriors.
BpPlan bp_plan(const GraphShape &g, int B, int iters, int algo, bool early_stop, bool mc, bool want_post, int cus);
// Whether the fixed-count decode of plan p (bp_loc_kernel) moves its rows 16 bytes at a time: n % 4
// = 0 (every local-edge layout's is), so row b of llr and post starts 16-byte aligned and row b of
// hard 4-byte aligned exactly when the tensor does; a null post or hard counts as aligned.
// Otherwise, or when narrow is set (LDPC_NO_WIDE_IO=1), 4-byte and 1-byte accesses.
bool bp_wide_io(const BpPlan &p, const GraphShape &g, bool early_stop, bool mc, const void *llr, const void *post,
                const void *hard, bool narrow);
// The plan of an ensemble call (bp_ens_kernel, bp_ens.hip): word b decodes on its own (dv, dc)
// regular graph, rows b of the sampler's two lists.  One workgroup owns one block
//   messages float[E] | channel LLRs float[n] | cross index int32[E]
// (E = n dv; ens_block_bytes, 16-byte padded) -- in LDS when it fits there beside the early-stop
// syndrome bits (ens_syn_bytes: two buffers of one bit per check, always in LDS) and the
// Monte-Carlo curve, otherwise in a slab of the scratch buffer, one per workgroup of the grid,
// with the first lds_slots messages kept in LDS.  dc > 32: BpPath::None.
BpPlan bp_ens_plan(int n, int dv, int dc, int B, int iters, int algo, bool early_stop, bool mc, bool want_post,
                   int cus);
// The plan of a layered (row-serial) call (bp_layer_kernel, bp_layer.hip) on a graph with a layer
// schedule (lay_L > 0; none: BpPath::None).  One workgroup owns one block
//   posteriors P float[n] | check->variable messages R float[E]
// (layer_block_bytes, 16-byte padded): wholly in LDS (256 threads, one workgroup per codeword)
// when it fits gmem_plan's budget beside the Monte-Carlo curve, otherwise in a slab of the
// scratch buffer, one per workgroup of the grid (1024 threads, one workgroup per CU), with the
// block's first lds_slots words -- P first -- kept in LDS.
BpPlan bp_layer_plan(const GraphShape &g, int B, int iters, int algo, bool early_stop, bool mc, bool want_post,
                     int cus);
// The plan of a fixed-point layered call (bp_layer_q_kernel, bp_layer_q.hip).  One workgroup (256
// threads, one per codeword) owns, after the 16-byte padded Monte-Carlo curve, the block
//   posteriors P int8[n], padded to 4 bytes | one record per check
// (layer_q_record_bytes: 4 bytes up to check degree 16, 8 up to 32) wholly in LDS.  There is no
// slab form: a block past gmem_plan's budget (160 KiB - 4 KiB) has no plan (BpPath::None), as has
// a graph without a layer schedule.  wg_per_cu: how many such workgroups one CU holds.
// A quasi-cyclic graph (qc_Z > 0) goes to bp_qc_q_kernel<T,MAXDC> (bp_qc_q.hip) with the same block,
// LDS formula and cap: T = 64 (one wave) when Z <= 64, else 256; MAXDC by the largest block-row degree.
BpPlan bp_layer_q_plan(const GraphShape &g, int B, int iters, int algo, bool early_stop, bool mc, bool want_post,
                       int cus);
// The same in the codeword mode (cw; Monte-Carlo only: no plan otherwise): after the records the
// block holds the codeword's bit plane of layer_q_plane_bytes(n).  A rate-matching description adds
// nothing: its count mask is re-read from the description.  Names, threads, grid and the cap are
// unchanged; wg_per_cu is that of the larger block.  cw = false is bp_layer_q_plan.
BpPlan bp_layer_q_cw_plan(const GraphShape &g, int B, int iters, bool mc, bool cw);
constexpr size_t layer_q_plane_bytes(size_t n) { return 4 * ((n + 31) / 32); }
constexpr size_t layer_q_record_bytes(int max_cdeg) { return max_cdeg <= 16 ? 4 : 8; }
constexpr size_t layer_block_bytes(size_t n, size_t E) { return pad16((n + E) * 4); }
// Row l of lay_tab: [j] (j <= 32) = first word of the layer's j-th edges in lay_var (and in R): the
// checks of a layer are sorted by falling degree, so position p of the layer has a j-th edge
// exactly when p < [j + 1] - [j] (and [1] - [0] is the layer's number of checks); [32] is the
// layer's end, the next row's [0].
constexpr int kLayerMaxD = 32, kLayerTab = kLayerMaxD + 1;
// Row r of qc_row (a quasi-cyclic code's block row r): [0] its degree d, then per edge j < d, in
// ascending block-column order, [1 + 2 j] the column base c Z and [2 + 2 j] the shift (0 past d).
constexpr int kQcRow = 1 + 2 * kLayerMaxD;
constexpr size_t ens_block_bytes(size_t n, size_t E) { return pad16(E * 8 + n * 4); }
// bp_generic_kernel's block: messages float[E] | channel LLRs float[n] | decision bytes u8[E]
constexpr size_t generic_block_bytes(size_t n, size_t E) { return pad16(E * 5 + n * 4); }
// The Monte-Carlo curve (iters + 1 counts) where something follows it in LDS: 16-byte padded
constexpr size_t curve_bytes(int iters) { return pad16((size_t)(iters + 1) * 4); }
constexpr size_t ens_syn_bytes(size_t m) { return pad16(2 * ((m + 31) / 32) * 4); }
// Compute units of the current device (256 when it cannot be queried), asked on every call:
// devices launch from their own host threads, and the slabs and the grid must agree per device.
int device_cus();

// The channel of a fused Monte-Carlo call (a member of the kernel argument structs, kernel_args.hpp)
struct ChanArgs {
    int kind;      // LDPC_CH_*
    float p, p2;   // see oracle_channel
    uint32_t k0, k1;
};
inline ChanArgs make_chan(int kind, float p, float p2, uint64_t seed) {
    ChanArgs c;
    c.kind = kind;
    c.p = p;
    c.p2 = p2;
    c.k0 = (uint32_t)seed;
    c.k1 = (uint32_t)(seed >> 32);
    return c;
}

// One soft-decoding call, whatever the family: what the C ABI's entries (capi.cpp) fill and the
// families below plan and launch from.  B > 0.
struct SoftCall {
    int B = 0, max_iters = 0, algo = 0;
    float alpha = 1.0f;
    bool early_stop = false;
    bool mc = false;  // fused-channel Monte-Carlo: ch / first_cw / trial / its; otherwise llr / post / hard / its
    const float *llr = nullptr;
    void *post = nullptr;  // float [B][n]; int8 for the fixed-point family; nullptr: no posteriors
    uint8_t *hard = nullptr;
    int32_t *its = nullptr;  // [B]
    bool narrow_io = false;  // LDPC_NO_WIDE_IO=1 (capi.cpp): no 16-byte row I/O (tests hold the wide path to the narrow one)
    ChanArgs ch{};
    uint64_t first_cw = 0;
    int32_t *trial = nullptr;  // [B][max_iters+1] per-trial curves (then launch_mc_reduce)
    // The codeword mode of the fixed-point family (mc only; ldpc_mc_layered_q_cw_batch_dev)
    bool cw_mode = false;
    const uint8_t *cw = nullptr;  // [B][n] codewords, bit 0; nullptr: all-zero
    const uint8_t *rm = nullptr;  // the rate-matching description's packed bytes; nullptr: none
    float known_llr = 0.0f;
};

// The soft-decoding families.  Each plans a call (its bp_*_plan, host only) and launches a plan
// it made: asynchronous on `s`, with plan.scratch bytes at `scratch` (capi.cpp's soft_launch has
// planned once, taken them from the workspace and refused a shorter buffer).  A call without a
// kernel: hipErrorInvalidValue from FloodFamily, hipErrorNotSupported from the others.
struct FloodFamily {  // flooding on a fixed code (bp_dispatch.hip and the kernel files behind it)
    const ldpc_graph &g;
    BpPlan plan(const SoftCall &c, int cus) const {
        BpPlan p = bp_plan(g, c.B, c.max_iters, c.algo, c.early_stop, c.mc, c.post != nullptr, cus);
        p.wide_io = bp_wide_io(p, g, c.early_stop, c.mc, c.llr, c.post, c.hard, c.narrow_io);
        return p;
    }
    hipError_t launch(const BpPlan &p, const SoftCall &c, float *scratch, hipStream_t s) const;
};
struct EnsFamily {  // word / trial b on graph b of the sampler's lists, int32 [B][n*dv] each, only read (bp_ens.hip)
    int n, dv, dc;
    const int32_t *chk, *var;
    BpPlan plan(const SoftCall &c, int cus) const {
        return bp_ens_plan(n, dv, dc, c.B, c.max_iters, c.algo, c.early_stop, c.mc, c.post != nullptr, cus);
    }
    hipError_t launch(const BpPlan &p, const SoftCall &c, float *scratch, hipStream_t s) const;
};
struct LayerFamily {  // layered (row-serial) schedule of graph_host.cpp's build_layer_schedule (bp_layer.hip)
    const ldpc_graph &g;
    BpPlan plan(const SoftCall &c, int cus) const {
        return bp_layer_plan(g, c.B, c.max_iters, c.algo, c.early_stop, c.mc, c.post != nullptr, cus);
    }
    hipError_t launch(const BpPlan &p, const SoftCall &c, float *scratch, hipStream_t s) const;
};
struct LayerQFamily {  // fixed-point layered min-sum (bp_layer_q.hip, bp_qc_q.hip); q validated by the caller; no scratch
    const ldpc_graph &g;
    const ldpc_quant &q;
    BpPlan plan(const SoftCall &c, int cus) const {
        if (c.cw_mode) return bp_layer_q_cw_plan(g, c.B, c.max_iters, c.mc, true);
        return bp_layer_q_plan(g, c.B, c.max_iters, 1, c.early_stop, c.mc, c.post != nullptr, cus);
    }
    hipError_t launch(const BpPlan &p, const SoftCall &c, float *scratch, hipStream_t s) const;
};

hipError_t launch_channel(int channel, float p, float p2, uint64_t seed, uint64_t first_cw, int n,
                          int B, void *d_out, hipStream_t stream);

// Monte-Carlo: a fused channel + decode writes per-trial curves into `trial` ([B][max_iters+1]
// int32) and its into `trial_its` ([B]); then the reducer.  launch_mc_bec (bec.hip): the erasure
// channel on a fixed code.
hipError_t launch_mc_bec(const ldpc_graph &g, float p, float p2, uint64_t seed, uint64_t first_cw, int B,
                         int max_iters, int32_t *trial, int32_t *trial_its, hipStream_t stream);
hipError_t launch_mc_reduce(const int32_t *trial, const int32_t *trial_its, int B, int max_iters,
                            int expurgation, int64_t stop_frame_errors, int64_t *d_counters,
                            int32_t *d_cutoff, hipStream_t stream);
// Gallager A/B (gb.hip), from a gb_plan of the same call: a decode of the words' bit 0 (hard, its:
// either may be nullptr), and the fused BSC channel + decode that fills trial and trial_its.
hipError_t launch_gb_decode(const GbPlan &p, const ldpc_graph &g, const uint8_t *d_bits, int B, int max_iters, int b,
                            bool early_stop, uint8_t *d_hard, int32_t *d_its, hipStream_t stream);
hipError_t launch_mc_gb(const GbPlan &p, const ldpc_graph &g, const ChanArgs &ch, uint64_t first_cw, int B,
                        int max_iters, int b, bool early_stop, int32_t *trial, int32_t *trial_its, hipStream_t stream);

// The launch plan of one encode call (encode_plan.cpp): encode_parity_kernel's tile width, grid
// and LDS and the parity-plane scratch, decided in one host-only function; encode.hip launches what
// it says.  One workgroup encodes a tile of 32 W codewords from the tile's K information planes in
// LDS (4 K W bytes); W is the widest of 4, 2, 1 whose planes fit kEncLdsCap.  threads == 0: they fit
// at no W.  A workgroup past half the CU's LDS is alone on its CU and takes 1,024 threads.
constexpr size_t kEncLdsCap = kLdsMax - 4096;
struct EncodePlan {
    const char *name = "none";  // display name, e.g. encode_parity_kernel<4>
    int threads = 0;
    int W = 0;               // plane words (of 32 codewords) per workgroup
    int cw_per_wg = 0;       // 32 W
    int64_t grid = 0;        // tiles: ceil(B / cw_per_wg)
    size_t lds = 0;          // dynamic LDS bytes
    size_t cap = 0;          // the cap `lds` was admitted under (kEncLdsCap)
    int64_t pwords = 0;      // plane words of a parity row: grid * W
    size_t scratch = 0;      // bytes of the parity planes uint32 [pwords][rank]
    int64_t write_grid = 0;  // workgroups (256 threads) of encode_write_kernel: one thread per 4 variables of a codeword
};
EncodePlan encode_plan(int n, int K, int rank, int B);

}  // namespace ldpc

// Device-resident systematic encoder (encode_host.hpp's description, uploaded): the handle of the
// C ABI's ldpc_encoder_* entries.
struct ldpc_encoder {
    int n = 0, K = 0, rank = 0, KW = 0, device = 0;
    std::vector<int32_t> info_pos, par_pos;  // host copies (ldpc_encoder_positions)
    uint32_t *At = nullptr;                  // [KW][rank] A transposed (encoder_device_tables)
    int32_t *src = nullptr;                  // [n] information index j, or ~i of parity row i
};

// Device-resident rate-matching description (rate_match_host.hpp's, uploaded): the handle of the C
// ABI's ldpc_rate_match_* entries.
struct ldpc_rate_match {
    int n = 0, n_tx = 0, n_punct = 0, n_known = 0, n_count = 0, device = 0;
    uint8_t *desc = nullptr;  // [4 ceil(n / 4)] packed bytes
};

namespace ldpc {

// The codeword family (encode.hip).  All asynchronous on `stream`.
// launch_encode: parity planes into `planes` (p.scratch bytes), then the codewords uint8 [B][n].
hipError_t launch_encode(const EncodePlan &p, const ldpc_encoder &e, const uint8_t *d_info, int B, uint32_t *planes,
                         uint8_t *d_cw, hipStream_t stream);
// Information bits uint8 [B][K] of trials first_cw .. first_cw + B - 1 (the header's info stream)
hipError_t launch_info_bits(uint64_t seed, uint64_t first_cw, int K, int B, uint8_t *d_info, hipStream_t stream);
// launch_channel's outputs reflected where the codeword bit is 1 (d_cw nullptr: all-zero)
hipError_t launch_channel_cw(int channel, float p, float p2, uint64_t seed, uint64_t first_cw, int n, int B,
                             const uint8_t *d_cw, void *d_out, hipStream_t stream);
// Per-trial rows for launch_mc_reduce: trial[b][0] = channel errors, trial[b][max_iters] = final
// errors against the codeword, the entries between them 0.
hipError_t launch_cw_count(const uint8_t *d_cw, const void *d_chan, bool chan_is_llr, const uint8_t *d_hard, int n,
                           int B, int max_iters, int32_t *trial, hipStream_t stream);

// Rate matching (rate_match.hip).  d_desc: the packed description (rate_match_host.hpp), 4-byte aligned.
// launch_channel_rm: launch_channel_cw's outputs at the transmitted positions, +0 / the erasure at the
// punctured ones, +-known_llr / the codeword bit at the known ones.
hipError_t launch_channel_rm(const uint8_t *d_desc, int channel, float p, float p2, float known_llr, uint64_t seed,
                             uint64_t first_cw, int n, int B, const uint8_t *d_cw, void *d_out, hipStream_t stream);
// launch_cw_count's rows under the description's classes and count mask (d_cw nullptr: all-zero);
// chan_kind 0: BEC words in d_chan and d_dec, 1: LLRs, 2: received bits.
hipError_t launch_rm_count(const uint8_t *d_desc, const uint8_t *d_cw, const void *d_chan, int chan_kind,
                           const uint8_t *d_dec, int n, int B, int max_iters, int32_t *trial, hipStream_t stream);

// Buckets (= threads per workgroup) of the parallel graph sampler for n*dv
// sockets; the permutation is in LDS (u16) when n*dv < 65536.  Must match
// oracle_sample_regular.
inline int sample_buckets(int E) { return E <= 16384 ? 256 : (E < 65536 ? 512 : 1024); }
// Sequential-draw sampler (sample_seq_kernel, one wave per graph) for
// kSeqMinE <= n*dv <= kSeqMaxE with check degrees <= kSeqMaxCdeg; the oracle's
// SEQ_* constants must equal these.  Larger graphs: one level, K = 1024.
constexpr int kSeqMinE = 8192, kSeqMaxE = 393216, kSeqMaxCdeg = 192;
// LDS of one sequential-draw attempt (sampler.hip asserts its carve against this): 344 words of
// sync words, retry lists and last pool entries, a ring of 512 entries of ring_bytes each (2: u16
// variable ids, 4: int), then the pool bitmap of bw words.
constexpr int kSeqThreads = 128, kSeqRingSlots = 512, kSeqFixedWords = 344;
constexpr size_t seq_plan_lds(int bw, int ring_bytes) {
    return (size_t)4 * ((size_t)bw + kSeqFixedWords) + (size_t)ring_bytes * kSeqRingSlots;
}

// The launch plan of one sampler call (sample_plan.cpp): which kernels run and everything their
// launches need, decided in one host-only function; sampler.hip launches what it says.
struct SamplePlan {
    bool seq = false;           // the sequential-draw sampler (else one Rao-Sandelius level)
    bool csr = false;           // irregular degree structure
    const char *draw = "none";  // sample_seq_kernel<regular|csr,u16|int> or sample_regular_kernel<K,u16|int32,lds|gmem>
    int threads = 0;            // of the draw kernel
    int K = 0;                  // one level: buckets (= threads); 0 for the sequential sampler
    size_t lds = 0;             // dynamic LDS bytes of the draw kernel (and of the search pass)
    int bw = 0;                 // sequential: bitmap words (a multiple of 4, 32 bw >= E)
    int ring = 0;               // sequential: bytes of a ring entry (2: u16 when n <= 65,536, else 4)
    int fb = 0;                 // sequential: bits of a variable's occurrence counter (0: max degree >= 256)
    int fbu = 0;                // fb when n counters fit the bitmap's LDS, else 0 (global CAS)
    int emit_fb = 0;            // what the emit pass is told: -1 (the variable-side kernel follows) or fbu
    uint32_t mdv = 0;           // regular: ceil(2^32 / dv) for socket / dv by multiply-high, 0: true divide
    const char *var_side = "none";  // sample_var_side_kernel<1024,u16|int32> when V > 0
    int V = 0;                  // variables per variable-side workgroup (a multiple of 64; 0: no such kernel)
    int nch = 0;                // chunks of V variables per graph
    int row = 0;                // bytes of a staged row entry (2: every check / slot id below 65,536, else 4)
    size_t vs_lds = 0;          // dynamic LDS bytes of the variable-side kernel
    const char *search = "none";    // sample_search_kernel<regular|csr,u16|int> when W > 0
    int per_cu = 0;             // search workgroups one CU holds (LDS bound)
    int W = 0;                  // persistent workgroups of the search pass (0: no search pass)
};
// (n, m, E): variables, checks, sockets; max_cdeg / max_vdeg: the largest degrees; regular: the
// (dv, dc) structure (dv is read only then); G graphs; cus: compute units of the device, 0 for
// the single-pass form without a search pass.
SamplePlan sample_plan(int n, int m, int E, int max_cdeg, int max_vdeg, bool regular, int dv, int G, int cus);

// Random regular graphs on the device (law of random_code_generator.c), one
// workgroup per graph; attempts[g] = number of permutations drawn (negative if
// max_attempts was hit without a valid graph).
// ctl: device scratch of sample_ctl_words(G) words for the sequential sampler's search pass
// (nullptr: the single-pass form, one wave draws a graph's attempts in order).
hipError_t launch_sample_regular(int n, int dv, int dc, uint64_t seed, uint64_t first_graph, int G,
                                 int32_t *check_lookup, int32_t *variable_lookup, int32_t *attempts,
                                 int max_attempts, uint32_t *ctl, hipStream_t stream);
inline size_t sample_ctl_words(int G) { return 2 + 4 * (size_t)G; }
// Diagnostics builds (-DLDPC_SEQ_STATS=1): the search and emit passes' per-phase counters
// (2 x kStCount words, see SeqStat in sampler.hip); hipErrorNotSupported in the product build.
hipError_t seq_stats(uint64_t *out, int reset);
// Irregular form: socket s of variable d_vsock[s]; check c owns slots [cptr[c], cptr[c+1]);
// outputs check_var[g][E] and var_slot[g][E] (CSR, each variable's slots ascending).
hipError_t launch_sample_csr(int n, int m, int E, const int32_t *d_vsock, const int32_t *d_cptr,
                             const int32_t *d_vptr, int max_cdeg, int max_vdeg, uint64_t seed, uint64_t first_graph,
                             int G, int32_t *check_var, int32_t *var_slot, int32_t *attempts, int max_attempts,
                             uint32_t *ctl, hipStream_t stream);
// Scan-path evidence of the peeling decoder (peel.hip; device global, this device): [0] overflowed
// iterations, [1] trials that overflowed, [2] trials decoded.
hipError_t peel_stats(uint64_t *out, int reset);
// Test-only cap on the peeling decoder's frontier-list capacity (F > 0), 0 restores the LDS
// budget's capacity.
void peel_cap(int F);
// BEC Monte-Carlo where trial b decodes on graph b of (check_lookup, variable_lookup): the
// frontier-peeling decoder (peel.hip) where its check state fits LDS, else bec_kernel.
hipError_t launch_mc_bec_ensemble(int n, int dv, int dc, const int32_t *check_lookup, const int32_t *variable_lookup,
                                  float p, uint64_t seed, uint64_t first_cw, int B, int max_iters, int32_t *trial,
                                  int32_t *trial_its, hipStream_t stream);

// ML ("optimal") erasure decoding, one workgroup per word (m <= 1000).
// cptr == nullptr: regular lists (check c = slots [c*dc, c*dc+dc)), word b reads
// cvar + b*cvar_stride.
hipError_t launch_ml_decode(const int32_t *cptr, const int32_t *cvar, int64_t cvar_stride, int dc, int n, int m,
                            const uint8_t *d_in, int B, uint8_t *d_out, int32_t *d_unsolved, hipStream_t stream);
// mc_reduce with a cutoff computed by an earlier launch_mc_reduce (trial_its may be null).
hipError_t launch_mc_reduce_cut(const int32_t *trial, const int32_t *trial_its, int B, int max_iters, int expurgation,
                                const int32_t *d_cutoff, int64_t *d_counters, hipStream_t stream);

// Kernel-choice introspection for tests / bench ("lds36", "generic", ...).
const char *bp_kernel_name(const ldpc_graph &g, int early_stop);

}  // namespace ldpc
