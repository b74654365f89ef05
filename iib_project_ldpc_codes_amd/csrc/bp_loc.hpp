// bp_loc_kernel: the local-edge soft decoder (layout: loc_layout.cpp), and its launch ladder.
// Included by bp_loc_spa.hip and bp_loc_ms.hip, which instantiate one algorithm each (the
// kernel's instantiations are most of the library's compile time).
#pragma once
#include "bp_loc_common.hpp"

namespace ldpc {
namespace {

// ---------------------------------------------------------------------------
// 2a'. Local-edge kernel (layout: loc_layout.cpp).  One codeword per workgroup of T
//   threads; thread t updates check pairs q = t + kT (k < KP) and the four variables
//   those checks hold as their local variables (var pairs 2k, 2k+1 on float2, .x = the
//   pair's first check side).  The local edge of each variable -- one per variable --
//   stays in a VGPR (loc[]) for the whole decode: the check phase reads it as input
//   slot s of check pair k and overwrites it with the check's output; the variable
//   phase reads that and overwrites it with the variable's extrinsic message.  Only the
//   other E - n messages live in LDS (rows per degree class, lane-contiguous
//   ds_read_b128 / ds_read_b64 on the check side, gathers on the variable side).
//   Sum-product in the product domain as bp_lds_kernel (R-wire, elementary-symmetric
//   check rule); min-sum in natural units, variable sums in variable_to_check_list order
//   (the local edge spliced in at its index) so it stays bit-exact with the oracle.
//   ABS: some variables have fewer than DVN+1 edges; their absent edges gather the
//   neutral value (ratio 1 / sum 0) and write to a private dummy word.
// ---------------------------------------------------------------------------

// code = dy, or dy | dx << 8 for a mixed pair (dx = dy - 1 = DHI - 1 only)
template <int D, int DHI, int ALGO, bool SGN>
__device__ __forceinline__ int loc_check_dispatch(int code, float *msg, int W, int Nc, int i, float2 &l0, float2 &l1,
                                                  float alpha, uint32_t lpar) {
    if constexpr (D == DHI) {
        if (code >> 8) return loc_check_pair<D, ALGO, true, SGN>(msg, W, Nc, i, l0, l1, alpha, lpar);
        return loc_check_pair<D, ALGO, false, SGN>(msg, W, Nc, i, l0, l1, alpha, lpar);
    } else {
        if (code == D) return loc_check_pair<D, ALGO, false, SGN>(msg, W, Nc, i, l0, l1, alpha, lpar);
        return loc_check_dispatch<D + 1, DHI, ALGO, SGN>(code, msg, W, Nc, i, l0, l1, alpha, lpar);
    }
}

// DVN0 / DVN1: non-local edges per variable of local slot 0 / 1 (max); ABS0 / ABS1: some
// variable of that slot has fewer (its absent edges gather the neutral value).
// MC (sum-product): fused Philox channel, per-iteration error counts of the all-zero
// codeword into the trial curve, no posteriors; ET with MC: syndrome early stop on the
// sign-bit decisions (see loc_check_pair).  ET without MC (hard-decision decodes: the caller
// asked for no posteriors): the same stop, the decisions of the stopping iteration kept in a
// bit per variable (hbits) and written out; a frame that never stops takes the fixed-count
// epilogue.
template <int DLO, int DHI, int DVN0, int DVN1, int KP, int T, int ALGO, bool ABS0, bool ABS1, bool ET = false,
          bool MC = false, bool EP = false>
__global__ __launch_bounds__(T, loc_waves_per_simd(T, KP)) void bp_loc_kernel(BpArgs a) {
    static_assert(!ET || ALGO == 0 || DLO == DHI, "min-sum early stop: one check class");
    static_assert(!ET || 2 * 2 * KP <= 64, "early stop keeps the thread's decisions in one 64-bit word");
    // MSET (min-sum Monte-Carlo with early stop): min-sum messages carry their own signs, so
    // the decisions cannot ride in them as in sum-product; instead every change of a
    // variable's decision XORs its checks' bits of an LDS syndrome (a few atomics once
    // decoding settles) and the next check phase tests that syndrome
    constexpr bool MSET = ET && ALGO == 1;
    constexpr bool SGN_LSB = ET && ALGO == 0;
    constexpr int VP = 2 * KP;  // variable pairs per thread
    constexpr int DVM = DVN0 > DVN1 ? DVN0 : DVN1;
    constexpr int DVA = DVM > 0 ? DVM : 1;
    constexpr int DVP = DVA;  // rows of loc_pos per var pair
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ uint32_t stop_flag[2];  // early stop: block_any's double-buffered flag
    float *msg = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x;
    const int n = a.n, iters = a.max_iters;
    const int lpos0 = (int)((uint32_t)(size_t)(lds_u8 *)smem >> 2);
    const uint32_t base2 = (uint32_t)lpos0 | ((uint32_t)lpos0 << 16);
    constexpr bool SPA = ALGO == 0;
    constexpr bool INF0 = ABS0 || ALGO == 1, INF1 = ABS1 || ALGO == 1;
    uint32_t sp[VP][DVA];
    uint32_t inf[VP];
    // packed LDS word pair of var pair v's non-local edge u (re-read per codeword and for
    // the posterior gathers: not held live outside the iteration loop, where the
    // staging and epilogue need the VGPRs).  The fixed-count decodes' table loads go by ld_row,
    // from a lane offset (lane_bytes) formed where the loads are
    auto lane_bytes = [&]() {
        uint32_t l = 4u * (uint32_t)tid;
        asm volatile("" : "+v"(l));
        return l;
    };
    auto load_sp = [&](int v, int u) { return (uint32_t)ld_fresh(a.loc_pos, (v * DVP + u) * T + tid) + base2; };
    // the variable ids of the thread's var pairs (entry 2v + h; -1: none), every load issued
    // before the first use (one L2 round trip, not one per var pair; Monte-Carlo staging)
    auto load_vars = [&](int (&vv)[2 * VP]) {
#pragma unroll
        for (int i = 0; i < 2 * VP; ++i) vv[i] = ld_fresh(a.loc_var, i * T + tid);
    };
    auto load_vars_row = [&](int (&vv)[2 * VP], uint32_t lane4) {
#pragma unroll
        for (int i = 0; i < 2 * VP; ++i) vv[i] = ld_row(row_rsrc(a.loc_var, 2 * VP * T * 4), i * T, lane4);
    };
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if constexpr (INF0) inf[2 * k] = (uint32_t)a.loc_info[(2 * k) * T + tid];
        if constexpr (INF1) inf[2 * k + 1] = (uint32_t)a.loc_info[(2 * k + 1) * T + tid];
    }
    auto at = [](uint32_t ba) -> lds_f32 & { return *(lds_f32 *)(size_t)ba; };
    const float neutral = SPA ? 1.0f : 0.0f;

    // gather the non-local c->v messages of var pair v (slot s) into cv[0 .. DN-1]
    auto gather = [&](auto dn_tag, auto abs_tag, int v, const uint32_t (&spv)[DVA], float2 (&cv)[DVA],
                      uint32_t (&a0)[DVA], uint32_t (&a1)[DVA]) {
        constexpr int DN = decltype(dn_tag)::value;
        constexpr bool AB = decltype(abs_tag)::value;
#pragma unroll
        for (int u = 0; u < DN; ++u) {
            a0[u] = pos_lo_x4(spv[u]);
            a1[u] = pos_hi_x4(spv[u]);
        }
#pragma unroll
        for (int u = 0; u < DN; ++u) cv[u] = make_float2(at(a0[u]), at(a1[u]));
        if constexpr (AB) {
#pragma unroll
            for (int u = 0; u < DN; ++u) {
                cv[u].x = (inf[v] >> u) & 1u ? cv[u].x : neutral;
                cv[u].y = (inf[v] >> (u + 4)) & 1u ? cv[u].y : neutral;
            }
        }
    };
    // min-sum posterior of var pair v: L + messages in variable_to_check_list order,
    // the local one spliced in at its index jl (the oracle's order: bit-exact)
    auto ms_sum = [&](auto dn_tag, int v, const float2 &Lv, const float2 &lv, const float2 (&cv)[DVA]) {
        constexpr int DN = decltype(dn_tag)::value;
        if constexpr (DN == 2) {
            // three terms in order: jl = 0 (ml, n0, n1), 1 (n0, ml, n1), 2 (n0, n1, ml); the masks
            // jl == 0 / jl == 2 are sign-extended one-hot bits of loc_info (v_bfe_i32), the
            // selects v_bfi_b32 -- VALU only, no per-lane masks held in SGPRs
            float s2[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t e0 = (uint32_t)__builtin_amdgcn_sbfe((int)inf[v], 16 + 4 * h, 1);
                const uint32_t e2 = (uint32_t)__builtin_amdgcn_sbfe((int)inf[v], 18 + 4 * h, 1);
                const uint32_t ml = __float_as_uint(h ? lv.y : lv.x);
                const uint32_t n0 = __float_as_uint(h ? cv[0].y : cv[0].x), n1 = __float_as_uint(h ? cv[1].y : cv[1].x);
                const float a0 = __uint_as_float(bfi_u32(e0, ml, n0));
                const uint32_t u = bfi_u32(e0, n0, ml);
                const float a1 = __uint_as_float(bfi_u32(e2, n1, u));
                const float a2 = __uint_as_float(bfi_u32(e2, ml, n1));
                s2[h] = (((h ? Lv.y : Lv.x) + a0) + a1) + a2;
            }
            return make_float2(s2[0], s2[1]);
        }
        float s2[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int jl = (inf[v] >> (8 + 2 * h)) & 3;
            const float ml = h ? lv.y : lv.x;
            float s = h ? Lv.y : Lv.x;
#pragma unroll
            for (int j = 0; j <= DN; ++j) {
                const float nl = j == 0 ? 0.0f : (h ? cv[j - 1].y : cv[j - 1].x);
                const float nl2 = j < DN ? (h ? cv[j].y : cv[j].x) : 0.0f;
                s += j < jl ? nl2 : (j == jl ? ml : nl);
            }
            s2[h] = s;
        }
        return make_float2(s2[0], s2[1]);
    };

    int *curve = reinterpret_cast<int *>(smem + (((size_t)(a.loc_words + 64 > n ? a.loc_words + 64 : n) * 4 + 15) &
                                                  ~(size_t)15));
    uint32_t *syn = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(curve) +
                                                 (((size_t)(iters + 1) * 4 + 15) & ~(size_t)15));
    const int nsw = (2 * a.loc_P + 31) >> 5;  // MSET: syndrome words (bit 2q + h: check h of pair q)
    // MSET / hard-decision ET: the thread's current decisions, bits 2v, 2v + 1 of var pair v
    using HB = std::conditional_t<(4 * KP > 32), uint64_t, uint32_t>;
    static_assert(!MSET || sizeof(HB) == 4, "MSET: 32-bit decision word");
    HB hbits = 0;
    HB lpar = 0;  // SGN: the parity of each check's two local decisions (see bits_parity)
    // MSET: the decisions that changed in a variable phase (chm, bit 2v + h: hbits before XOR
    // after) flip the syndrome bits of their checks -- the local one (pair q = tid + (v/2) T, bit
    // 2q + h) and the non-local ones (from the slot's packed LDS positions, re-read from L2:
    // a select chain over the register copies measured 15 % slower).
    // Each lane walks its own marks after the phase, so the wave loops max-over-lanes times
    // instead of running a var pair's flips whenever one lane of the wave changed it.
    uint32_t chm = 0u;
    auto syn_flush = [&]() {
        uint32_t mk = chm;
        chm = 0u;
        const uint32_t P4 = 4u * (uint32_t)a.loc_P;
        constexpr int NF = 2;  // flips per trip (1: -0.4 %, 4: -1.5 %, profiles/r05_ab_flip_batch_locvar.txt)
        while (__builtin_amdgcn_ballot_w64(mk != 0u)) {
            // NF flips per trip: every flip's non-local positions loaded before the first use
            // (one L2 round trip per NF flips; rows u < DVM exist for every var pair, so the
            // loads need no guard), the 16-bit half by a bit-field extract (no branch)
            int bit[NF];
            bool on[NF];
            uint32_t raw[NF][DVA];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                bit[f] = mk ? (int)__builtin_ctz(mk) : 0;
                on[f] = mk != 0u && tid + (bit[f] >> 2) * T < a.loc_P;  // var pair v = bit / 2, pair slot v / 2
                mk &= mk - 1u;
            }
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int u = 0; u < DVM; ++u) raw[f][u] = (uint32_t)a.loc_pos[((bit[f] >> 1) * DVP + u) * T + tid];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                if (on[f]) {
                    const int v = bit[f] >> 1, h = bit[f] & 1;
                    const int q = tid + (v >> 1) * T;
                    const uint32_t bl = 2u * (uint32_t)q + (uint32_t)h;
                    atomicXor(&syn[bl >> 5], 1u << (bl & 31));
                    const int dn = (v & 1) ? DVN1 : DVN0;
#pragma unroll
                    for (int u = 0; u < DVM; ++u) {
                        if (u < dn) {
                            uint32_t w = __builtin_amdgcn_ubfe(raw[f][u], 16u * (uint32_t)h, 16u);
                            w = w >= P4 ? w - P4 : w;
                            const uint32_t bn = 2u * (w >> 2) + (w & 1u);
                            atomicXor(&syn[bn >> 5], 1u << (bn & 31));
                        }
                    }
                }
            }
        }
    };
    // EP (early stop, posteriors asked for): a persistent grid takes codewords from a global
    // counter (frames stop at different iterations) and keeps each variable pair's product of
    // incoming c->v ratios (min-sum: its posterior sum) of the latest variable phase in the
    // workgroup's slab, a.scratch + blockIdx.x * VP * T float2 (lane-contiguous stores, L2-
    // resident: 40 KB per workgroup); the stopping iteration's posteriors come from there.
    // The slab is written only in variable phases that follow a check phase with at most
    // LDPC_LOC_EP_W0 threads holding an unsatisfied check (frames converge through nearly
    // satisfied syndromes); a frame that stops without a slab from its last variable phase
    // is decoded again from its channel LLRs -- the same deterministic trajectory -- with
    // the slab written in that variable phase (redo_it).
    static_assert(!EP || (ET && !MC), "EP: early-stop decodes with posteriors");
    constexpr bool ep = EP;
    float2 *slab = ep ? reinterpret_cast<float2 *>(a.scratch) + (size_t)blockIdx.x * VP * T : nullptr;
    // persistent grid (a.work: EP, and early stop without posteriors when LDPC_LOC_PERSIST):
    // codewords come from a global counter; thread 0 claims the next one a codeword ahead, so
    // the atomic's latency hides behind the current decode
    __shared__ int next_b;
    const bool per = a.work != nullptr;
    uint32_t claim = 0u;
    for (int round = 0;; ++round) {
        if (per && tid == 0) next_b = round == 0 ? (int)atomicAdd(a.work, 1u) : (int)claim;
        __syncthreads();  // the previous codeword's outputs are out of LDS; next_b visible
        const int b = per ? __builtin_amdgcn_readfirstlane(next_b) : (int)blockIdx.x + round * (int)gridDim.x;
        if (b >= a.B) break;
        if (per && tid == 0) claim = atomicAdd(a.work, 1u);
        const uint64_t cw = a.first_cw + (uint64_t)b;
        int redo_it = -1;  // EP: the variable phase whose slab a second pass must write
    restart:
        int slab_it = -2;  // EP: the variable phase that last wrote the slab
        bool slab_now = false;
        if constexpr (ET) {
            if (tid == 0) stop_flag[0] = stop_flag[1] = 0u;  // visible after the staging barrier
        }
        // the table loads follow the LLR copy (batched before it: neutral to 0.5 % slower)
        auto load_tabs = [&]() {
#pragma unroll
            for (int k = 0; k < KP; ++k) {
#pragma unroll
                for (int u = 0; u < DVN0; ++u) sp[2 * k][u] = load_sp(2 * k, u);
#pragma unroll
                for (int u = 0; u < DVN1; ++u) sp[2 * k + 1][u] = load_sp(2 * k + 1, u);
            }
        };
        int vv[2 * VP];
        int err0 = 0;
        if constexpr (MC) {
            for (int i = tid; i <= iters; i += T) curve[i] = 0;
            if constexpr (MSET)
                for (int i = tid; i < nsw; i += T) syn[i] = 0u;
            for (int g4 = tid; g4 < (n + 3) >> 2; g4 += T) {  // one Philox block per four variables
                const uint4 r = chan_block(a.ch, cw, g4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (4 * g4 + q >= n) break;
                    const float l = chan_soft_word(a.ch, r, q);
                    msg[4 * g4 + q] = to_msg<ALGO>(l);
                    err0 += (l < 0.0f);
                }
            }
        } else {
            if constexpr (MSET)
                for (int i = tid; i < nsw; i += T) syn[i] = 0u;
            for (int v = tid; v < n; v += T) msg[v] = to_msg<ALGO>(a.llr[(size_t)b * n + v]);
        }
        __syncthreads();
        if constexpr (MC) {
            const int w = wave_sum(err0);
            if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[0], w);
        }
        load_tabs();
        float2 L[VP];  // SPA: E = 2^channel (clamped); min-sum: channel LLR
        if constexpr (MC) {
            load_vars(vv);
#pragma unroll
            for (int v = 0; v < VP; ++v)
                L[v] = make_float2(vv[2 * v] >= 0 ? msg[vv[2 * v]] : 0.0f, vv[2 * v + 1] >= 0 ? msg[vv[2 * v + 1]] : 0.0f);
        } else {
#pragma unroll
            for (int v = 0; v < VP; ++v) {
                const int v0 = ld_fresh(a.loc_var, (v * 2 + 0) * T + tid), v1 = ld_fresh(a.loc_var, (v * 2 + 1) * T + tid);
                L[v] = make_float2(v0 >= 0 ? msg[v0] : 0.0f, v1 >= 0 ? msg[v1] : 0.0f);
            }
        }
        __syncthreads();
        float2 loc[VP];
        auto init = [&](auto dn_tag, int v) {
            constexpr int DN = decltype(dn_tag)::value;
            float2 w;
            if constexpr (SPA) {
                w = make_float2(__builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(L[v].x, -23.0f, 23.0f)),
                                __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(L[v].y, -23.0f, 23.0f)));
                if constexpr (ET)  // the channel decision in the LSB
                    w = make_float2(__uint_as_float(bfi_lsb(__float_as_uint(w.x), (uint32_t)(L[v].x < 0.0f))),
                                    __uint_as_float(bfi_lsb(__float_as_uint(w.y), (uint32_t)(L[v].y < 0.0f))));
                L[v] = make_float2(__builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(L[v].x, -126.0f, 126.0f)),
                                   __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(L[v].y, -126.0f, 126.0f)));
            } else {
                w = L[v];
                if constexpr (MSET) {  // the channel decisions' syndrome
                    const int d0 = (int)(w.x < 0.0f) | ((int)(w.y < 0.0f) << 1);
                    hbits |= (uint32_t)d0 << (2 * v);
                    chm |= (uint32_t)d0 << (2 * v);
                }
            }
            loc[v] = w;
#pragma unroll
            for (int u = 0; u < DN; ++u) {
                at(pos_lo_x4(sp[v][u])) = w.x;
                at(pos_hi_x4(sp[v][u])) = w.y;
            }
        };
        hbits = 0u;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            init(int_c<DVN0>{}, 2 * k);
            init(int_c<DVN1>{}, 2 * k + 1);
        }
        if constexpr (MSET) syn_flush();
        // variable phase of var pair v; returns the pair's hard decisions (bit 0: .x, 1: .y)
        auto var_pair = [&](auto dn_tag, auto abs_tag, int v) -> int {
            constexpr int DN = decltype(dn_tag)::value;
            constexpr int DV = DN + 1;
            uint32_t a0[DVA], a1[DVA];
            float2 cv[DVA];
            gather(dn_tag, abs_tag, v, sp[v], cv, a0, a1);
            int dec = 0;
            if constexpr (SPA) {
                // edges e_0 = local, e_{1+u} = non-local u: R_j = E prod_{k != j} e_k
                float2 pre[DV];
                pre[0] = L[v];
                if constexpr (DV > 1) pre[1] = pre[0] * loc[v];
#pragma unroll
                for (int j = 2; j < DV; ++j) pre[j] = pre[j - 1] * cv[j - 2];
                uint32_t sx = 0, sy = 0;  // ET: the decision rides in every outgoing mantissa LSB
                if constexpr (MC || ET) {
                    // P < 1 on the bits: P is a product of positive clamped ratios, so
                    // bits(P) - bits(1.0) is negative exactly when P < 1 (no compare / select)
                    const float2 P = DN > 0 ? pre[DV - 1] * cv[DN > 0 ? DN - 1 : 0] : pre[DV - 1];
                    const uint32_t dx = (__float_as_uint(P.x) + 0xC0800000u) >> 31;
                    const uint32_t dy = (__float_as_uint(P.y) + 0xC0800000u) >> 31;
                    dec = (int)(dx | dy << 1);
                    if constexpr (ET) {
                        sx = dx;
                        sy = dy;
                    }
                }
                auto sgn = [&](float2 R) {
                    if constexpr (ET)  // LSB := decision (one v_bfi_b32 per value)
                        return make_float2(__uint_as_float(bfi_lsb(__float_as_uint(R.x), sx)),
                                           __uint_as_float(bfi_lsb(__float_as_uint(R.y), sy)));
                    return R;
                };
                float2 suf = DN > 0 ? cv[DN > 0 ? DN - 1 : 0] : make_float2(1.0f, 1.0f);
#pragma unroll
                for (int j = DV - 1; j >= 1; --j) {
                    const float2 R = sgn(ratio_wire2(j == DV - 1 ? pre[j] : pre[j] * suf));
                    at(a0[j - 1]) = R.x;
                    at(a1[j - 1]) = R.y;
                    if (j < DV - 1) suf = suf * cv[j - 1];
                }
                if (ep && slab_now) slab[v * T + tid] = loc[v] * suf;  // prod of the incoming c->v ratios
                loc[v] = ratio_wire2(DN > 0 ? L[v] * suf : L[v]);  // local edge: its decision is in lpar
            } else {
                const float2 s = ms_sum(dn_tag, v, L[v], loc[v], cv);
                if (ep && slab_now) slab[v * T + tid] = s;  // the posterior itself
#pragma unroll
                for (int u = 0; u < DN; ++u) {
                    at(a0[u]) = s.x - cv[u].x;
                    at(a1[u]) = s.y - cv[u].y;
                }
                loc[v] = make_float2(s.x - loc[v].x, s.y - loc[v].y);
                // decisions from the sign bits: a min-sum posterior is never -0 (see to_msg)
                if constexpr (MC || ET)
                    dec = (int)((__float_as_uint(s.x) >> 31) | ((__float_as_uint(s.y) >> 31) << 1));
            }
            return dec;
        };
        int it = 0;
        bool stopped = false;
        for (; it < iters; ++it) {
            __syncthreads();  // variable phase (or initialisation) complete
            int unsat = 0;
            {  // the gathers' unpacked addresses stay in the loop
#pragma unroll
                for (int v = 0; v < VP; ++v)
#pragma unroll
                    for (int u = 0; u < DVA; ++u)
                        asm volatile("" : "+v"(sp[v][u]));
            }
            if constexpr (ALGO == 1) {  // the order masks (ms_sum) are re-derived per iteration, not held
#pragma unroll
                for (int v = 0; v < VP; ++v) asm volatile("" : "+v"(inf[v]));
            }
            // ---- check phase ----
            if (LDPC_LOC_PRIO) __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                int q = tid + k * T;
                asm volatile("" : "+v"(q));  // recomputed per iteration: no per-pair addresses held live
                if (q < a.loc_P) {
                    if constexpr (DLO == DHI) {  // one class: rows of P pairs from word 0
                        unsat |= loc_check_pair<DLO, ALGO, false, ET && SPA>(msg, 0, a.loc_P, q, loc[2 * k],
                                                                             loc[2 * k + 1], a.alpha,
                                                                             (uint32_t)(lpar >> (4 * k)));
                    } else {
                        // class of q by selects on the (scalar) class table -- no per-lane
                        // indexing of kernel arguments
                        int q0 = a.loc_cls_q[0], q1 = a.loc_cls_q[1], W = a.loc_cls_w[0], d = a.loc_cls_d[0];
#pragma unroll
                        for (int j = 1; j < 4; ++j) {
                            const bool in = j < a.loc_ncls && q >= a.loc_cls_q[j];
                            q0 = in ? a.loc_cls_q[j] : q0;
                            q1 = in ? a.loc_cls_q[j + 1] : q1;
                            W = in ? a.loc_cls_w[j] : W;
                            d = in ? a.loc_cls_d[j] : d;
                        }
                        unsat |= loc_check_dispatch<DLO, DHI, ALGO, ET && SPA>(d, msg, W, q1 - q0, q - q0, loc[2 * k],
                                                                               loc[2 * k + 1], a.alpha,
                                                                               (uint32_t)(lpar >> (4 * k)));
                    }
                }
                if (LDPC_LOC_CGROUP > 0 && k % LDPC_LOC_CGROUP == LDPC_LOC_CGROUP - 1)
                    __builtin_amdgcn_sched_barrier(0);  // pairs in flight (VGPR budget)
            }
            if constexpr (MSET)
                for (int i = tid; i < nsw; i += T) unsat |= syn[i] != 0u;
            if constexpr (ET) {
                // the syndrome of the previous variable phase's decisions: stop when every
                // check is satisfied (oracle: after that iteration)
                if constexpr (SGN_LSB) unsat &= 1;  // the parities are in bit 0 of the OR of the pairs' words
                bool more;
                if constexpr (EP) {
                    const uint32_t cnt = block_count(unsat | (it == 0), stop_flag, it & 1);
                    more = cnt != 0u;
                    slab_now = cnt <= (uint32_t)LDPC_LOC_EP_W0 || it == redo_it;
                    if (more && slab_now) slab_it = it;
                } else {
                    more = block_any(unsat | (it == 0), stop_flag, it & 1);
                }
                if (!more) {
                    stopped = true;
                    break;
                }
            } else {
                __syncthreads();
            }
            if (!MC && it == iters - 1) break;  // the last variable phase only forms posteriors
            // ---- variable phase ----
            if (LDPC_LOC_PRIO) __builtin_amdgcn_s_setprio(1);
            int errs = 0;
            HB nh = 0;  // early stop: this phase's decisions, bits 2v, 2v + 1
            {
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    const int d0 = var_pair(int_c<DVN0>{}, bool_c<ABS0>{}, 2 * k);
                    if (LDPC_LOC_VGROUP == 1) __builtin_amdgcn_sched_barrier(0);
                    const int d1 = var_pair(int_c<DVN1>{}, bool_c<ABS1>{}, 2 * k + 1);
                    if (LDPC_LOC_VGROUP > 0) __builtin_amdgcn_sched_barrier(0);
                    if constexpr (ET) nh |= (HB)(d0 | d1 << 2) << (4 * k);
                    else if constexpr (MC) errs += tid + k * T < a.loc_P ? __builtin_popcount(d0) + __builtin_popcount(d1) : 0;
                }
            }
            if constexpr (ET) {
                if constexpr (MSET) chm = (uint32_t)(nh ^ hbits);
                hbits = nh;
                if constexpr (SGN_LSB) lpar = nh ^ (nh >> 2);  // bit 4k (+1): check 2q (+1)'s local parity
                if constexpr (MC) {  // pair slots k with tid + k T < P hold variables
                    const int lim = a.loc_P - tid, nk = lim <= 0 ? 0 : min(KP, (lim + T - 1) / T);
                    const HB vm = 4 * nk >= 8 * (int)sizeof(HB) ? ~(HB)0 : (((HB)1 << (4 * nk)) - 1);
                    errs = sizeof(HB) == 8 ? __builtin_popcountll((uint64_t)(nh & vm)) : __builtin_popcount((uint32_t)(nh & vm));
                }
                if constexpr (MSET) syn_flush();
            }
            if constexpr (MC) {
                const int w = wave_sum(errs);
                if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[it + 1], w);
            }
        }
        if constexpr (MC) {
            __syncthreads();
            int32_t *tr = a.trial + (size_t)b * (iters + 1);
            const int last = curve[it];
            for (int i = tid; i <= iters; i += T) tr[i] = i <= it ? curve[i] : last;
            if (tid == 0) a.its[b] = it;
            continue;
        }
        if constexpr (ET && !MC) {
            if (stopped && ep && slab_it != it - 1) {  // no slab from the last variable phase: again
                redo_it = it - 1;
                __syncthreads();  // every thread is past its reads of this pass's LDS
                goto restart;
            }
            if (stopped && ep) {
                // posteriors of the stopping iteration from the slab (its last variable phase):
                // SPA log2 E + log2(prod c->v) -- the oracle's L + sum of the c->v messages -- and
                // the decisions that satisfied every check (hbits) as the hard decisions; staged
                // through LDS (posteriors in words [0, n), decision bytes after them: the messages
                // are dead once the stop is known)
                uint8_t *hb = reinterpret_cast<uint8_t *>(msg + n);
#pragma unroll
                for (int v = 0; v < VP; ++v) {
                    const float2 q = slab[v * T + tid];
                    float2 pv;
                    if constexpr (SPA) {
                        pv = make_float2(__builtin_amdgcn_logf(L[v].x) + __builtin_amdgcn_logf(q.x),
                                         __builtin_amdgcn_logf(L[v].y) + __builtin_amdgcn_logf(q.y));
                    } else {
                        pv = q;
                    }
                    const int v0 = ld_fresh(a.loc_var, (v * 2 + 0) * T + tid), v1 = ld_fresh(a.loc_var, (v * 2 + 1) * T + tid);
                    if constexpr (SPA) {  // a clamped E (|LLR| > 87 nats): the channel value itself
                        const float lx = __builtin_amdgcn_logf(L[v].x), ly = __builtin_amdgcn_logf(L[v].y);
                        if (v0 >= 0 && fabsf(lx) >= 125.5f) pv.x = to_msg<ALGO>(a.llr[(size_t)b * n + v0]) + __builtin_amdgcn_logf(q.x);
                        if (v1 >= 0 && fabsf(ly) >= 125.5f) pv.y = to_msg<ALGO>(a.llr[(size_t)b * n + v1]) + __builtin_amdgcn_logf(q.y);
                    }
                    if (v0 >= 0) {
                        msg[v0] = pv.x;
                        hb[v0] = (uint8_t)((hbits >> (2 * v)) & 1);
                    }
                    if (v1 >= 0) {
                        msg[v1] = pv.y;
                        hb[v1] = (uint8_t)((hbits >> (2 * v + 1)) & 1);
                    }
                }
                __syncthreads();
                for (int v = tid; v < n; v += T) {
                    a.post[(size_t)b * n + v] = msg[v] * Domain<ALGO>::out;
                    if (a.hard) a.hard[(size_t)b * n + v] = hb[v];
                }
                if (a.its && tid == 0) a.its[b] = it;
                continue;
            }
        }
        if constexpr (ET) {
            if (stopped) {  // hard decisions of the stopping iteration (no posteriors asked for)
#pragma unroll
                for (int v = 0; v < VP; ++v) {
                    const int v0 = ld_fresh(a.loc_var, (v * 2 + 0) * T + tid), v1 = ld_fresh(a.loc_var, (v * 2 + 1) * T + tid);
                    if (v0 >= 0) msg[v0] = (hbits >> (2 * v)) & 1 ? -1.0f : 1.0f;
                    if (v1 >= 0) msg[v1] = (hbits >> (2 * v + 1)) & 1 ? -1.0f : 1.0f;
                }
                __syncthreads();
                if (a.hard)
                    for (int v = tid; v < n; v += T) a.hard[(size_t)b * n + v] = (uint8_t)(msg[v] < 0.0f);
                if (a.its && tid == 0) a.its[b] = it;
                continue;
            }
        }
        // ---- posteriors (after the last check phase) and outputs ----
        // (variable ids re-read where needed: not kept live through the decode loop)
        // Fixed-count decodes (FIX) make one pass over the tables here: the gathers take the
        // loop's own packed positions (sp[][], still in registers), each variable id is loaded
        // once (pid[], issued before the gathers: used only behind the barrier), and the clamped-E
        // test is made once, a ballot over the thread's values: a wave that holds one (rare) takes
        // the pass that substitutes the channel values (SUBST), the others a pass without the
        // test.  The other decodes read the tables again per var pair.
        constexpr bool FIX = !ET && !MC;
        float2 pr[VP];
        int pid[2 * VP];
        bool clamped = false;
        if constexpr (FIX) {
            load_vars_row(pid, lane_bytes());
            if constexpr (SPA) {
#pragma unroll
                for (int v = 0; v < VP; ++v)
                    clamped |= fabsf(__builtin_amdgcn_logf(L[v].x)) >= 125.5f || fabsf(__builtin_amdgcn_logf(L[v].y)) >= 125.5f;
            }
        }
        auto post = [&](auto dn_tag, auto abs_tag, auto subst_tag, int v) {
            constexpr int DN = decltype(dn_tag)::value;
            constexpr bool SUBST = decltype(subst_tag)::value;
            uint32_t a0[DVA], a1[DVA], spv[DVA];
            float2 cv[DVA];
            if constexpr (FIX) {
                gather(dn_tag, abs_tag, v, sp[v], cv, a0, a1);
            } else {
#pragma unroll
                for (int u = 0; u < DN; ++u) spv[u] = load_sp(v, u);
                gather(dn_tag, abs_tag, v, spv, cv, a0, a1);
            }
            if constexpr (SPA) {
                float2 s;
                // the channel term from the register-held E = 2^L: log2 E is L to ~1e-7 (no
                // second 40 KB read of the codeword's LLRs); a clamped E (|LLR| > 87 nats) takes
                // the input value itself
                s = make_float2(__builtin_amdgcn_logf(L[v].x), __builtin_amdgcn_logf(L[v].y));
                if constexpr (FIX) {
                    if constexpr (SUBST) {
                        const float *lb = a.llr + (size_t)b * n;
                        if (fabsf(s.x) >= 125.5f && pid[2 * v] >= 0) s.x = to_msg<ALGO>(lb[pid[2 * v]]);
                        if (fabsf(s.y) >= 125.5f && pid[2 * v + 1] >= 0) s.y = to_msg<ALGO>(lb[pid[2 * v + 1]]);
                    }
                } else if (fabsf(s.x) >= 125.5f || fabsf(s.y) >= 125.5f) {
                    const float *lb = a.llr + (size_t)b * n;
                    const int v0 = ld_fresh(a.loc_var, (v * 2 + 0) * T + tid);
                    const int v1 = ld_fresh(a.loc_var, (v * 2 + 1) * T + tid);
                    if (fabsf(s.x) >= 125.5f && v0 >= 0) s.x = to_msg<ALGO>(lb[v0]);
                    if (fabsf(s.y) >= 125.5f && v1 >= 0) s.y = to_msg<ALGO>(lb[v1]);
                }
                s = s + make_float2(__builtin_amdgcn_logf(loc[v].x), __builtin_amdgcn_logf(loc[v].y));
#pragma unroll
                for (int u = 0; u < DN; ++u)
                    s = s + make_float2(__builtin_amdgcn_logf(cv[u].x), __builtin_amdgcn_logf(cv[u].y));
                pr[v] = s;
            } else {
                pr[v] = ms_sum(dn_tag, v, L[v], loc[v], cv);
            }
            __builtin_amdgcn_sched_barrier(0);  // one var pair's gathers in flight (VGPR budget)
        };
        if (FIX && SPA && __builtin_expect(__builtin_amdgcn_ballot_w64(clamped) != 0, 0)) {
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                post(int_c<DVN0>{}, bool_c<ABS0>{}, bool_c<true>{}, 2 * k);
                post(int_c<DVN1>{}, bool_c<ABS1>{}, bool_c<true>{}, 2 * k + 1);
            }
        } else {
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                post(int_c<DVN0>{}, bool_c<ABS0>{}, bool_c<false>{}, 2 * k);
                post(int_c<DVN1>{}, bool_c<ABS1>{}, bool_c<false>{}, 2 * k + 1);
            }
        }
        __syncthreads();  // all gathers done before the staging overwrites messages
        if constexpr (FIX) {  // an absent variable (-1) writes the spare word behind variable n - 1
#pragma unroll
            for (int v = 0; v < VP; ++v) {
                msg[min((uint32_t)pid[2 * v], (uint32_t)n)] = pr[v].x;
                msg[min((uint32_t)pid[2 * v + 1], (uint32_t)n)] = pr[v].y;
            }
        } else {
#pragma unroll
            for (int v = 0; v < VP; ++v) {
                const int v0 = ld_fresh(a.loc_var, (v * 2 + 0) * T + tid);
                const int v1 = ld_fresh(a.loc_var, (v * 2 + 1) * T + tid);
                if (v0 >= 0) msg[v0] = pr[v].x;
                if (v1 >= 0) msg[v1] = pr[v].y;
            }
        }
        __syncthreads();
        if constexpr (FIX) {
            // n <= 2 VP T; the rows go through their descriptors (row_rsrc), the lane's part one 32-bit byte
            // offset: every LDS read
            // issued before the first store, a read past variable n - 1 takes the spare words and its
            // store is dropped.  wide_io: 16 bytes of posteriors and four packed decisions a store
            uint32_t t = (uint32_t)tid;
            asm volatile("" : "+v"(t));  // as ld_fresh: no index per entry held across the decode
            if (a.wide_io) {
                f32x4 o[VP / 2];
#pragma unroll
                for (int j = 0; j < VP / 2; ++j)
                    o[j] = *reinterpret_cast<const f32x4 *>(msg + min(4u * (t + j * T), (uint32_t)n));
                if (a.post) {
                    const __amdgpu_buffer_rsrc_t rp = row_rsrc(a.post + (size_t)b * n, 4 * n);
#pragma unroll
                    for (int j = 0; j < VP / 2; ++j)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o[j] * Domain<ALGO>::out), rp,
                                                               16u * (t + j * T), 0, 0);
                }
                if (a.hard) {
                    const __amdgpu_buffer_rsrc_t rh = row_rsrc(a.hard + (size_t)b * n, n);
#pragma unroll
                    for (int j = 0; j < VP / 2; ++j) {
                        const uint32_t h = (uint32_t)(o[j].x < 0.0f) | (uint32_t)(o[j].y < 0.0f) << 8 |
                                           (uint32_t)(o[j].z < 0.0f) << 16 | (uint32_t)(o[j].w < 0.0f) << 24;
                        __builtin_amdgcn_raw_buffer_store_b32(h, rh, 4u * (t + j * T), 0, 0);
                    }
                }
            } else {
                float o[2 * VP];
#pragma unroll
                for (int i = 0; i < 2 * VP; ++i) o[i] = msg[min(t + i * T, (uint32_t)n)];
                if (a.post) {
                    const __amdgpu_buffer_rsrc_t rp = row_rsrc(a.post + (size_t)b * n, 4 * n);
#pragma unroll
                    for (int i = 0; i < 2 * VP; ++i)
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[i] * Domain<ALGO>::out), rp,
                                                              4u * (t + i * T), 0, 0);
                }
                if (a.hard) {
                    const __amdgpu_buffer_rsrc_t rh = row_rsrc(a.hard + (size_t)b * n, n);
#pragma unroll
                    for (int i = 0; i < 2 * VP; ++i)
                        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(o[i] < 0.0f), rh, t + i * T, 0, 0);
                }
            }
        } else {
            for (int v = tid; v < n; v += T) {
                const float s = msg[v];
                if (a.post) a.post[(size_t)b * n + v] = s * Domain<ALGO>::out;
                if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(s < 0.0f);
            }
        }
        if (a.its && tid == 0) a.its[b] = iters;
    }
}

// bp_loc_chain.hpp (included by bp_loc_spa.hip only): bp_loc_chain_kernel<KP, T, ...> and its launcher
template <int KP, int T>
hipError_t launch_loc_chain(const BpPlan &p, const ldpc_graph &g, BpArgs a, hipStream_t s);

// bp_loc_kernel shapes: (check-degree range, non-local edges per variable, absent edges)
// x (threads, check pairs per thread)
template <int DLO, int DHI, int D0, int D1, bool A0, bool A1, int T, int KP, int ALGO, bool ET, bool MC>
hipError_t launch_loc_shape(const BpPlan &p, BpArgs a, hipStream_t s) {
    auto launch = [&](auto k) {
        if (p.persistent) {  // the grid pulls codewords from a counter
            a.work = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(a.scratch) + p.counter);
            const hipError_t e = hipMemsetAsync(a.work, 0, sizeof(uint32_t), s);
            if (e != hipSuccess) return e;
        }
        return launch_lds(k, dim3(p.grid), dim3(T), p.lds, s, a);
    };
    if constexpr (ET && !MC) {  // early stop with posteriors: per-workgroup slabs before the counter
        if (a.post) return launch(bp_loc_kernel<DLO, DHI, D0, D1, KP, T, ALGO, A0, A1, true, false, true>);
    }
    return launch(bp_loc_kernel<DLO, DHI, D0, D1, KP, T, ALGO, A0, A1, ET, MC>);
}

// The instantiations of a variant: its rows of the shape table (kernel_shapes.hpp), the ones
// loc_variant admits the variant for
template <int DLO, int DHI, int D0, int D1, bool A0, bool A1, int ALGO, bool ET, bool MC>
hipError_t launch_loc_deg(const BpPlan &p, const BpArgs &a, int T, int KP, hipStream_t s) {
#define LDPC_ROW(TT, KK) \
    if (T == TT && KP == KK) return launch_loc_shape<DLO, DHI, D0, D1, A0, A1, TT, KK, ALGO, ET, MC>(p, a, s);
    LDPC_LOC_SHAPES(LDPC_ROW)
    if constexpr (DLO != DHI) {
        LDPC_LOC_RSU_SHAPES(LDPC_ROW)
    } else {
        LDPC_LOC_REG36_SHAPES(LDPC_ROW)
    }
#undef LDPC_ROW
    return hipErrorInvalidValue;
}

template <int ALGO, bool ET, bool MC>
hipError_t launch_loc_modes(const BpPlan &p, const ldpc_graph &g, BpArgs a, hipStream_t s) {
    if (p.chain) {  // the chained layout: a kernel and a launcher of its own, fixed-count sum-product only
        if constexpr (ALGO == 0 && !ET && !MC) return launch_loc_chain<kLocChainKP, kLocChainT>(p, g, a, s);
        else return hipErrorInvalidValue;
    }
    a.loc_var = g.loc_var;
    a.loc_pos = g.loc_pos;
    a.loc_info = g.loc_info;
    a.loc_P = g.loc_P;
    a.loc_ncls = g.loc_ncls;
    a.loc_words = g.loc_words;
    for (int i = 0; i < 5; ++i) {
        a.loc_cls_q[i] = g.loc_cls_q[i];
        a.loc_cls_w[i] = g.loc_cls_w[i];
    }
    for (int i = 0; i < 4; ++i) a.loc_cls_d[i] = g.loc_cls_d[i];
    // the template family from the whole layout shape (loc_variant), not the degrees alone
    const int variant = loc_variant(g.loc_dlo, g.loc_dhi, g.loc_DVN, g.loc_dvn0, g.loc_dvn1, g.loc_abs0, g.loc_abs1,
                                    g.loc_T, g.loc_KP);
    if (variant == kLocReg36) return launch_loc_deg<6, 6, 2, 2, false, false, ALGO, ET, MC>(p, a, g.loc_T, g.loc_KP, s);
    if (variant == kLocNone) return hipErrorInvalidValue;
    if constexpr (ET && ALGO == 1) return hipErrorInvalidValue;  // min-sum early stop: one check class only
    else return launch_loc_deg<5, 6, 1, 3, false, true, ALGO, ET, MC>(p, a, g.loc_T, g.loc_KP, s);
}

template <int ALGO>
hipError_t launch_loc_algo(const BpPlan &p, const ldpc_graph &g, const BpArgs &a, bool et, bool mc, hipStream_t s) {
    if (mc) return et ? launch_loc_modes<ALGO, true, true>(p, g, a, s) : launch_loc_modes<ALGO, false, true>(p, g, a, s);
    return et ? launch_loc_modes<ALGO, true, false>(p, g, a, s) : launch_loc_modes<ALGO, false, false>(p, g, a, s);
}

}  // namespace
}  // namespace ldpc
