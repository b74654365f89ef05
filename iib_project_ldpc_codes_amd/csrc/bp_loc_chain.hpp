// bp_loc_chain_kernel: the fixed-count sum-product decode of a (3,6) code on the chained local-edge layout
// (build_loc_chain_layout, loc_layout.cpp), and its launcher.  Included by bp_loc_spa.hip only.
// It shares with bp_loc_kernel (bp_loc.hpp) the layout family and what bp_loc_common.hpp holds -- the check
// rule of a check pair, the row and table loads -- and nothing else: no mode, algorithm or degree is a
// parameter here.  The variable update and the posterior sum are written out in both kernels, in one operation
// order: as functions called by both they missed their timing on two bp_loc_kernel shapes.  No
// test ties the two copies to each other -- the layouts' outputs differ in the last bits by design -- so a
// change to one has to be made to the other by hand.
#pragma once
#include "bp_loc_common.hpp"

namespace ldpc {
namespace {

// One codeword per workgroup, launched Tq threads wide (n = 4 KP Tq).  Thread t owns the check pairs
// t + k Tq, k < KP, and the four variables each of them holds as its local variables (var pairs 2k, 2k + 1
// on float2).  Per variable one edge is local (loc[], a register for the whole decode) and two are not:
//   - pair slot 0 reads its four other inputs from two float4 rows of Tq pairs at word 0;
//   - pair slot k >= 1 takes input slot 2 from the chain register chain[k - 1] and its three others from a
//     float4 and a float2 row of (KP - 1) Tq pairs, behind slot 0's rows (word 8 Tq);
//   - var pair 2k + 1, k < KP - 1, sends its last edge to chain[k] and gathers the other from LDS (row 0 of
//     loc_pos); every other var pair gathers and scatters both.
// No lane tests tid < Tq: every thread of the launch holds all KP pair slots and all of its 4 KP variables, a
// part-filled last wave is the hardware's EXEC mask, and what the workgroup does together strides by Tq.
// T is the stride of the thread-layout tables (loc_var, loc_pos) and the launch bound.
// TQ > 0 (a row of LDPC_LOC_CHAIN_TQ, kernel_shapes.hpp): Tq as a compile-time constant -- n, the row bases,
// the class sizes and the copies' strides fold, and the check phase's row offsets are instruction immediates.
// TQ = 0: Tq = a.loc_cls_q[1], the row base a.loc_cls_w[1].  The launcher starts either only on a plan of its width.
template <int KP, int T, int TQ>
__global__ __launch_bounds__(T, loc_waves_per_simd(T, KP)) void bp_loc_chain_kernel(BpArgs a) {
    static_assert(TQ <= T, "a compile-time width is a launch width");
    constexpr int CL = KP - 1;   // chain links per thread
    constexpr int VP = 2 * KP;   // variable pairs per thread
    constexpr int D = 6, DN = 2; // check degree; non-local edges per variable (rows of loc_pos per var pair)
    // var pair v's last non-local edge is the chain register chain[v / 2]
    auto chained = [](int v) { return (v & 1) && (v >> 1) < CL; };
    float2 chain[CL];
    extern __shared__ __align__(16) unsigned char smem[];
    float *msg = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x;
    const int n = TQ > 0 ? 4 * KP * TQ : a.n, iters = a.max_iters;
    const int Tq = TQ > 0 ? TQ : a.loc_cls_q[1];
    const int lpos0 = (int)((uint32_t)(size_t)(lds_u8 *)smem >> 2);
    const uint32_t base2 = (uint32_t)lpos0 | ((uint32_t)lpos0 << 16);
    // packed LDS word pair of var pair v's non-local edge u (a chained var pair has no second one), and the
    // variable ids of the thread's var pairs (entry 2v + h).  Read per codeword, by ld_row from a lane
    // offset formed where the loads are: nothing per entry is held outside the iteration loop, where the
    // staging and epilogue need the VGPRs
    uint32_t sp[VP][DN];
    auto lane_bytes = [&]() {
        uint32_t l = 4u * (uint32_t)tid;
        asm volatile("" : "+v"(l));
        return l;
    };
    auto load_sp = [&](int v, int u, uint32_t lane4) {
        return (uint32_t)ld_row(row_rsrc(a.loc_pos, VP * DN * T * 4), (v * DN + u) * T, lane4) + base2;
    };
    auto load_vars_row = [&](int (&vv)[2 * VP], uint32_t lane4) {
#pragma unroll
        for (int i = 0; i < 2 * VP; ++i) vv[i] = ld_row(row_rsrc(a.loc_var, 2 * VP * T * 4), i * T, lane4);
    };
    auto at = [](uint32_t ba) -> lds_f32 & { return *(lds_f32 *)(size_t)ba; };
    // the non-local c->v messages of var pair v into cv[]: from LDS, a chained pair's last from its chain register
    auto gather = [&](int v, const uint32_t (&spv)[DN], float2 (&cv)[DN], uint32_t (&a0)[DN], uint32_t (&a1)[DN]) {
        const int nl = chained(v) ? DN - 1 : DN;
#pragma unroll
        for (int u = 0; u < DN; ++u)
            if (u < nl) {
                a0[u] = pos_lo_x4(spv[u]);
                a1[u] = pos_hi_x4(spv[u]);
            }
#pragma unroll
        for (int u = 0; u < DN; ++u)
            if (u < nl) cv[u] = make_float2(at(a0[u]), at(a1[u]));
        if (chained(v)) cv[DN - 1] = chain[v >> 1];
    };
    // the plan may size the grid below B: workgroup x takes codewords x, x + grid, ...
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        __syncthreads();  // the previous codeword's outputs are out of LDS
        // ---- staging: every table load (L2) is issued before the LLR copy (HBM), so the two latencies overlap ----
        {
            const uint32_t lane4 = lane_bytes();
#pragma unroll
            for (int k = 0; k < KP; ++k) {
#pragma unroll
                for (int u = 0; u < DN; ++u) sp[2 * k][u] = load_sp(2 * k, u, lane4);
#pragma unroll
                for (int u = 0; u < DN; ++u)
                    if (!(chained(2 * k + 1) && u == DN - 1)) sp[2 * k + 1][u] = load_sp(2 * k + 1, u, lane4);
            }
        }
        int vv[2 * VP];
        load_vars_row(vv, lane_bytes());
        {
            // every variable is the local one of one check and every thread holds 2 VP of them, so
            // n = 2 VP Tq: the copy is 2 VP loads per thread, all in flight at once (one HBM round
            // trip), striding by the launch width, and covers the row exactly -- nothing is read or
            // staged past variable n - 1.  The rows go through their descriptor (row_rsrc); group j's
            // offset j Tq is the instruction's scalar offset (as ld_row's entry), the lane's part one
            // 32-bit byte offset.  wide_io (the plan: rows 16-byte aligned): VP / 2 groups of four
            // consecutive variables, 16 bytes a load and an LDS write
            const __amdgpu_buffer_rsrc_t rl = row_rsrc(a.llr + (size_t)b * n, 4 * n);
            uint32_t t = (uint32_t)tid;
            asm volatile("" : "+v"(t));  // as ld_fresh: no index per entry held across the decode
            if (a.wide_io) {
                f32x4 r[VP / 2];
#pragma unroll
                for (int j = 0; j < VP / 2; ++j)
                    r[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rl, 16u * t, 16 * j * Tq, 0));
#pragma unroll
                for (int j = 0; j < VP / 2; ++j) {
                    f32x4 w;
                    w.x = to_msg<0>(r[j].x); w.y = to_msg<0>(r[j].y);
                    w.z = to_msg<0>(r[j].z); w.w = to_msg<0>(r[j].w);
                    *reinterpret_cast<f32x4 *>(msg + 4u * (t + (uint32_t)(j * Tq))) = w;
                }
            } else {
                float r[2 * VP];
#pragma unroll
                for (int i = 0; i < 2 * VP; ++i)
                    r[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rl, 4u * t, 4 * i * Tq, 0));
#pragma unroll
                for (int i = 0; i < 2 * VP; ++i) msg[t + (uint32_t)(i * Tq)] = to_msg<0>(r[i]);
            }
        }
        __syncthreads();
        float2 L[VP];  // E = 2^channel (clamped at 2^+-126)
#pragma unroll
        for (int v = 0; v < VP; ++v) L[v] = make_float2(msg[vv[2 * v]], msg[vv[2 * v + 1]]);
        __syncthreads();
        // ---- initialisation: every edge carries its variable's channel ratio ----
        float2 loc[VP];
#pragma unroll
        for (int v = 0; v < VP; ++v) {
            // the wire value clamp(E, 2^-23, 2^23) from the one E = exp2(clamp(L, +-126)): v_exp_f32
            // is monotone and exact at +-23, so this is exp2(clamp(L, +-23)) to the bit
            // (scripts/diag/fixed_cost_probe.hip compares the two over every float)
            L[v] = make_float2(__builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(L[v].x, -126.0f, 126.0f)),
                               __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(L[v].y, -126.0f, 126.0f)));
            const float2 w = make_float2(__builtin_amdgcn_fmed3f(L[v].x, 0x1p-23f, 0x1p23f),
                                         __builtin_amdgcn_fmed3f(L[v].y, 0x1p-23f, 0x1p23f));
            loc[v] = w;
#pragma unroll
            for (int u = 0; u < DN; ++u) {
                if (chained(v) && u == DN - 1) {
                    chain[v >> 1] = w;
                } else {
                    at(pos_lo_x4(sp[v][u])) = w.x;
                    at(pos_hi_x4(sp[v][u])) = w.y;
                }
            }
        }
        auto var_pair = [&](int v) {
            uint32_t a0[DN], a1[DN];
            float2 cv[DN];
            gather(v, sp[v], cv, a0, a1);
            // edges e_0 = local, e_{1+u} = non-local u: R_j = E prod_{k != j} e_k, from prefix products taken up
            // the edges and a suffix product taken down them (bp_loc_kernel's order: the two stay bit-exact)
            constexpr int DV = DN + 1;
            float2 pre[DV];
            pre[0] = L[v];
            pre[1] = pre[0] * loc[v];
#pragma unroll
            for (int j = 2; j < DV; ++j) pre[j] = pre[j - 1] * cv[j - 2];
            float2 suf = cv[DN - 1];
#pragma unroll
            for (int j = DV - 1; j >= 1; --j) {
                const float2 R = ratio_wire2(j == DV - 1 ? pre[j] : pre[j] * suf);
                if (chained(v) && j == DV - 1) {
                    chain[v >> 1] = R;
                } else {
                    at(a0[j - 1]) = R.x;
                    at(a1[j - 1]) = R.y;
                }
                if (j < DV - 1) suf = suf * cv[j - 1];
            }
            loc[v] = ratio_wire2(L[v] * suf);
        };
        for (int it = 0; it < iters; ++it) {
            __syncthreads();  // variable phase (or initialisation) complete
            {  // the gathers' unpacked addresses stay in the loop
#pragma unroll
                for (int v = 0; v < VP; ++v)
#pragma unroll
                    for (int u = 0; u < DN; ++u)
                        if (!(chained(v) && u == DN - 1)) asm volatile("" : "+v"(sp[v][u]));
            }
            // ---- check phase (VALU-bound: wave priority 0, see LDPC_LOC_PRIO) ----
            if (LDPC_LOC_PRIO) __builtin_amdgcn_s_setprio(0);
            // slots k >= 1: rows behind slot 0's two float4 rows of Tq pairs (the launcher passes the same word)
            const int W1 = TQ > 0 ? 8 * TQ : a.loc_cls_w[1];
            // TQ: the last row access, slot KP - 1's float2 row, is the immediate 4 (W1 + 16 Tq + 2 (KP - 2) Tq)
            // = 120 Tq bytes behind its lane base, within a ds_* instruction's 16-bit offset (the kernel has
            // no static LDS: the dynamic segment starts at 0)
            static_assert(4 * (8 * TQ + 4 * (KP - 1) * TQ + 2 * (KP - 2) * TQ) <= 65535,
                          "the chained rows' offsets are instruction immediates");
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                // the pair is entry i + off of its rows.  TQ: the slot's part is a constant, so every row of
                // the phase is a lane base (16 tid or 8 tid bytes, loop-invariant and held in a register
                // each) plus an immediate; else the index is recomputed per iteration (no per-pair address held)
                const int off = TQ > 0 && k > 0 ? (k - 1) * TQ : 0;
                int i = TQ > 0 ? tid : tid + (k > 0 ? (k - 1) * Tq : 0);
                if constexpr (TQ == 0) asm volatile("" : "+v"(i));
                if (k == 0)
                    loc_check_pair<D, 0>(msg, 0, Tq, i, loc[0], loc[1], a.alpha);
                else
                    loc_check_pair<D, 0, false, false, CL>(msg, W1, (KP - 1) * Tq, i, loc[2 * k], loc[2 * k + 1],
                                                           a.alpha, 0u, &chain[k - 1], off);
                if (LDPC_LOC_CGROUP > 0 && k % LDPC_LOC_CGROUP == LDPC_LOC_CGROUP - 1)
                    __builtin_amdgcn_sched_barrier(0);  // pairs in flight (VGPR budget)
            }
            __syncthreads();
            if (it == iters - 1) break;  // the last variable phase only forms posteriors
            // ---- variable phase (LDS-bound: wave priority 1) ----
            if (LDPC_LOC_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                var_pair(2 * k);
                if (LDPC_LOC_VGROUP == 1) __builtin_amdgcn_sched_barrier(0);
                var_pair(2 * k + 1);
                if (LDPC_LOC_VGROUP > 0) __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- posteriors (after the last check phase) and outputs ----
        // One pass over the tables: the gathers take the loop's own packed positions (sp[][], still in
        // registers), each variable id is loaded once (pid[], issued before the gathers: used only behind
        // the barrier), and the clamped-E test is made once, a ballot over the thread's values: a wave that
        // holds one (rare) takes the pass that substitutes the channel values, the others a pass without the test
        float2 pr[VP];
        int pid[2 * VP];
        bool clamped = false;
        load_vars_row(pid, lane_bytes());
#pragma unroll
        for (int v = 0; v < VP; ++v)
            clamped |= fabsf(__builtin_amdgcn_logf(L[v].x)) >= 125.5f || fabsf(__builtin_amdgcn_logf(L[v].y)) >= 125.5f;
        auto post = [&](bool subst, int v) {
            uint32_t a0[DN], a1[DN];
            float2 cv[DN];
            gather(v, sp[v], cv, a0, a1);
            // the channel term from the register-held E = 2^L: log2 E is L to ~1e-7 (no second 40 KB read of
            // the codeword's LLRs); a clamped E (|LLR| > 87 nats) takes the input value itself
            float2 s = make_float2(__builtin_amdgcn_logf(L[v].x), __builtin_amdgcn_logf(L[v].y));
            if (subst) {
                const float *lb = a.llr + (size_t)b * n;
                if (fabsf(s.x) >= 125.5f && pid[2 * v] >= 0) s.x = to_msg<0>(lb[pid[2 * v]]);
                if (fabsf(s.y) >= 125.5f && pid[2 * v + 1] >= 0) s.y = to_msg<0>(lb[pid[2 * v + 1]]);
            }
            s = s + make_float2(__builtin_amdgcn_logf(loc[v].x), __builtin_amdgcn_logf(loc[v].y));
#pragma unroll
            for (int u = 0; u < DN; ++u) s = s + make_float2(__builtin_amdgcn_logf(cv[u].x), __builtin_amdgcn_logf(cv[u].y));
            pr[v] = s;
            __builtin_amdgcn_sched_barrier(0);  // one var pair's gathers in flight (VGPR budget)
        };
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(clamped) != 0, 0)) {
#pragma unroll
            for (int v = 0; v < VP; ++v) post(true, v);
        } else {
#pragma unroll
            for (int v = 0; v < VP; ++v) post(false, v);
        }
        __syncthreads();  // all gathers done before the staging overwrites messages
#pragma unroll
        for (int v = 0; v < VP; ++v) {
            msg[pid[2 * v]] = pr[v].x;
            msg[pid[2 * v + 1]] = pr[v].y;
        }
        __syncthreads();
        {
            // n = 2 VP Tq (see the LLR copy): the same strides by the launch width cover the rows exactly,
            // group j's offset the stores' scalar offset; every LDS read issued before the first store
            uint32_t t = (uint32_t)tid;
            asm volatile("" : "+v"(t));  // as ld_fresh: no index per entry held across the decode
            if (a.wide_io) {
                f32x4 o[VP / 2];
#pragma unroll
                for (int j = 0; j < VP / 2; ++j)
                    o[j] = *reinterpret_cast<const f32x4 *>(msg + 4u * (t + (uint32_t)(j * Tq)));
                if (a.post) {
                    const __amdgpu_buffer_rsrc_t rp = row_rsrc(a.post + (size_t)b * n, 4 * n);
#pragma unroll
                    for (int j = 0; j < VP / 2; ++j)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o[j] * Domain<0>::out), rp,
                                                               16u * t, 16 * j * Tq, 0);
                }
                if (a.hard) {
                    const __amdgpu_buffer_rsrc_t rh = row_rsrc(a.hard + (size_t)b * n, n);
#pragma unroll
                    for (int j = 0; j < VP / 2; ++j) {
                        const uint32_t h = (uint32_t)(o[j].x < 0.0f) | (uint32_t)(o[j].y < 0.0f) << 8 |
                                           (uint32_t)(o[j].z < 0.0f) << 16 | (uint32_t)(o[j].w < 0.0f) << 24;
                        __builtin_amdgcn_raw_buffer_store_b32(h, rh, 4u * t, 4 * j * Tq, 0);
                    }
                }
            } else {
                float o[2 * VP];
#pragma unroll
                for (int i = 0; i < 2 * VP; ++i) o[i] = msg[t + (uint32_t)(i * Tq)];
                if (a.post) {
                    const __amdgpu_buffer_rsrc_t rp = row_rsrc(a.post + (size_t)b * n, 4 * n);
#pragma unroll
                    for (int i = 0; i < 2 * VP; ++i)
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[i] * Domain<0>::out), rp, 4u * t,
                                                              4 * i * Tq, 0);
                }
                if (a.hard) {
                    const __amdgpu_buffer_rsrc_t rh = row_rsrc(a.hard + (size_t)b * n, n);
#pragma unroll
                    for (int i = 0; i < 2 * VP; ++i)
                        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(o[i] < 0.0f), rh, t, i * Tq, 0);
                }
            }
        }
        if (a.its && tid == 0) a.its[b] = iters;
    }
}

// The chained layout's tables and its two row classes (pair slot 0 | the chained slots) into the arguments, and
// the launch: p.width threads.  The kernel strides by the launch width and tests no lane, so the width must
// be Tq and the rows 4 KP Tq long; anything else is refused and nothing is launched.
template <int KP, int T>
hipError_t launch_loc_chain(const BpPlan &p, const ldpc_graph &g, BpArgs a, hipStream_t s) {
    if (g.chn_Tq <= 0 || g.chn_Tq > T || g.loc_P != KP * g.chn_Tq || !g.chn_var || !g.chn_pos ||
        p.width != g.chn_Tq || a.n != 4 * KP * g.chn_Tq)
        return hipErrorInvalidValue;
    a.loc_var = g.chn_var;
    a.loc_pos = g.chn_pos;
    a.loc_info = g.chn_info;
    a.loc_P = g.loc_P;
    a.loc_ncls = 2;
    a.loc_words = g.chn_words;
    a.loc_cls_q[0] = 0; a.loc_cls_q[1] = g.chn_Tq; a.loc_cls_q[2] = g.loc_P;
    a.loc_cls_w[0] = 0; a.loc_cls_w[1] = 8 * g.chn_Tq; a.loc_cls_w[2] = g.chn_words;
    a.loc_cls_d[0] = a.loc_cls_d[1] = 6;
    // a plan with a compile-time width (BpPlan::tq): that row's instantiation, which takes Tq, n and the
    // row bases from its template argument -- started on no other width
    if (p.tq != 0) {
        if (p.tq != g.chn_Tq) return hipErrorInvalidValue;
#define LDPC_ROW(TQ) \
    if (p.tq == TQ) return launch_lds(bp_loc_chain_kernel<KP, T, TQ>, dim3(p.grid), dim3(p.width), p.lds, s, a);
        LDPC_LOC_CHAIN_TQ(LDPC_ROW)
#undef LDPC_ROW
        return hipErrorInvalidValue;
    }
    return launch_lds(bp_loc_chain_kernel<KP, T, 0>, dim3(p.grid), dim3(p.width), p.lds, s, a);
}

}  // namespace
}  // namespace ldpc
