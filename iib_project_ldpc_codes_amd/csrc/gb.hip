// Gallager A/B hard-decision decoding on the BSC, bit-sliced: gb_kernel and its launchers.
//
// The decoder is the one include/ldpc_mi355x.h defines ("Gallager A/B"); tests/gallager_ref.py
// restates it.  Every message is one bit, so a plane word of P carries the same message of
// BITS = 8 sizeof(P) codewords: bit i of a plane word is codeword i of the workgroup, as in
// bec.hip's bit-sliced kernels.
//
// LDS of a workgroup (gb_plan.cpp sizes it):
//   M[E]  one plane word per slot, check-slot order.  The check phase turns a check's slots from
//         v->c into c->v in place (T = XOR of its slots, slot ^= T); the variable phase gathers
//         its d slots through vslot and writes the new v->c bits back in place.
//   Y[n]  the received planes.
//   X[n]  the decision planes (early stop and Monte-Carlo only; a fixed-count decode writes its
//         last iteration's decisions over Y, which nothing reads afterwards).
//   cnt[BITS]  Monte-Carlo: the weight of x per codeword.  flag[3]: "some check unsatisfied" planes.
//
// Variable rule: D = number of disagreeing messages as four carry-save planes (d <= 15), then
// G1 = [D >= b_d], G2 = [D >= b_d + 1], GX = [D >= (d + 3) / 2] (2 D > d + 1) by a bitwise
// comparator against the per-variable constants; output j = y ^ (G2 | (G1 & ~dis_j)), x = y ^ GX.
//
// Early stop: the syndrome of x after iteration t is gathered through cvar by the check phase of
// iteration t + 1 (the last iteration needs none: its = max_iters either way).  A codeword whose
// syndrome is zero leaves the `active` plane; its bits of X, its count and its `its` are frozen
// from then on while the other codewords of the plane word go on in lockstep -- M and the
// comparisons of a stopped codeword still run, nothing reads them.  The workgroup ends once no
// codeword is active.
#include "kernel_args.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {
namespace {

// [count >= k] per bit column, count = c3 c2 c1 c0 (planes), 1 <= k <= 15
__device__ __forceinline__ uint32_t planes_ge(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, int k) {
    const uint32_t c[4] = {c0, c1, c2, c3};
    uint32_t gt = 0u, eq = ~0u;
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        const uint32_t ki = (k >> i) & 1 ? ~0u : 0u;
        gt |= eq & c[i] & ~ki;
        eq &= ~(c[i] ^ ki);
    }
    return gt | eq;
}

// dis added into the four-plane carry-save count
__device__ __forceinline__ void planes_add(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t dis) {
    const uint32_t k0 = c0 & dis;
    c0 ^= dis;
    const uint32_t k1 = c1 & k0;
    c1 ^= k0;
    const uint32_t k2 = c2 & k1;
    c2 ^= k1;
    c3 ^= k2;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x |= (uint32_t)__shfl_xor((int)x, off, kWave);
    return x;
}

// The variable update of one variable of degree d in slots vs[e0 .. e0 + d): new v->c planes into
// M, returns x.  D > 0: d == D at compile time (the slots and their messages stay in registers).
template <typename P, int D>
__device__ __forceinline__ uint32_t gb_variable(P *M, const int32_t *vs, int e0, int d, uint32_t y, int b) {
    uint32_t c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
    const int bd = b == 0 ? d - 1 : min(b, d - 1);
    if constexpr (D > 0) {
        int s[D];
        uint32_t dis[D];
#pragma unroll
        for (int j = 0; j < D; ++j) s[j] = vs[e0 + j];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            dis[j] = (uint32_t)M[s[j]] ^ y;
            planes_add(c0, c1, c2, c3, dis[j]);
        }
        const uint32_t g1 = planes_ge(c0, c1, c2, c3, bd), g2 = planes_ge(c0, c1, c2, c3, bd + 1);
#pragma unroll
        for (int j = 0; j < D; ++j) M[s[j]] = (P)(y ^ (g2 | (g1 & ~dis[j])));
    } else {
        for (int e = e0; e < e0 + d; ++e) planes_add(c0, c1, c2, c3, (uint32_t)M[vs[e]] ^ y);
        if (d >= 2) {
            const uint32_t g1 = planes_ge(c0, c1, c2, c3, bd), g2 = planes_ge(c0, c1, c2, c3, bd + 1);
            for (int e = e0; e < e0 + d; ++e) {
                const int s = vs[e];
                const uint32_t dis = (uint32_t)M[s] ^ y;
                M[s] = (P)(y ^ (g2 | (g1 & ~dis)));
            }
        } else if (d == 1) {
            M[vs[e0]] = (P)y;
        }
    }
    return y ^ planes_ge(c0, c1, c2, c3, (d + 3) >> 1);
}

template <int T, typename P, bool ES, bool MC>
__global__ __launch_bounds__(T) void gb_kernel(GbArgs a) {
    static_assert(T % 64 == 0, "lane groups of BITS codewords tile the waves");
    constexpr int BITS = 8 * sizeof(P);  // codewords per plane word and per workgroup
    constexpr bool HASX = ES || MC;
    constexpr uint32_t FULL = BITS == 32 ? ~0u : (1u << BITS) - 1u;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int n = a.n, m = a.m, E = a.E, iters = a.max_iters, B = a.B;
    P *M = reinterpret_cast<P *>(smem);  // [E]
    P *Y = M + E;                        // [n]
    P *X = HASX ? Y + n : Y;             // [n]
    int *cnt = reinterpret_cast<int *>(smem + ((((size_t)E + (HASX ? 2 : 1) * (size_t)n) * sizeof(P) + 15) & ~(size_t)15));  // [BITS]
    uint32_t *flag = reinterpret_cast<uint32_t *>(cnt + BITS);  // [3]
    const int64_t b0 = (int64_t)blockIdx.x * BITS;
    const int nloc = (int)min((int64_t)BITS, (int64_t)B - b0);  // codewords of this workgroup with rows
    uint32_t act = nloc >= 32 ? ~0u : (1u << nloc) - 1u;       // the same value in every thread
    int its = iters;                                           // of codeword tid (tid < nloc)

    if (tid < BITS) cnt[tid] = 0;
    if (tid < 3) flag[tid] = 0u;
    if (MC) __syncthreads();
    // ---- received planes ----
    if constexpr (MC) {
        // a group of BITS lanes = one group of 4 variables; lane = codeword bit (bec_mc_bits_kernel's draw)
        const int ngr = (n + 3) >> 2;
        const int bit = tid & (BITS - 1);
        const int shift = lane & ~(BITS - 1);
        const uint64_t cw = a.first_cw + (uint64_t)(b0 + bit);
        int local = 0;
        for (int g0 = 0; g0 < ngr; g0 += T / BITS) {  // every lane of a wave takes every ballot
            const int g = g0 + tid / BITS;
            const uint4 r = philox_block((uint32_t)g, 0u, (uint32_t)cw, (uint32_t)(cw >> 32), a.ch.k0, a.ch.k1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = 4 * g + j;
                const bool flip = v < n && u01(pick4(r, j)) < a.ch.p;  // the BSC stream: LLR < 0
                const uint64_t bal = __ballot(flip);
                local += flip;
                if (bit == 0 && v < n) {
                    const P w = (P)(bal >> shift);
                    Y[v] = w;
                    X[v] = w;
                }
            }
        }
        if (local) atomicAdd(&cnt[bit], local);
    } else {
        for (int v = tid; v < n; v += T) {
            uint32_t w = 0u;
            for (int i = 0; i < nloc; ++i) w |= (uint32_t)(a.bits[(size_t)(b0 + i) * n + v] & 1u) << i;
            Y[v] = (P)w;
            if (HASX) X[v] = (P)w;
        }
    }
    __syncthreads();
    for (int s = tid; s < E; s += T) M[s] = Y[a.cvar[s]];
    if (MC && tid < nloc) a.trial[(size_t)(b0 + tid) * (iters + 1)] = cnt[tid];
    __syncthreads();

    int t = 1;
    for (; t <= iters; ++t) {
        // ---- check phase: v->c into c->v in place; the syndrome of the previous decisions ----
        uint32_t unsat = 0u;
        for (int c = tid; c < m; c += T) {
            const int s0 = a.dc > 0 ? c * a.dc : a.cptr[c];
            const int s1 = a.dc > 0 ? s0 + a.dc : a.cptr[c + 1];
            uint32_t tot = 0u, syn = 0u;
            for (int s = s0; s < s1; ++s) {
                tot ^= M[s];
                if (ES && t > 1) syn ^= X[a.cvar[s]];
            }
            for (int s = s0; s < s1; ++s) M[s] = (P)((uint32_t)M[s] ^ tot);
            unsat |= syn;
        }
        if (ES && t > 1) {
            unsat = wave_or(unsat);
            if (lane == 0 && unsat) atomicOr(&flag[t % 3], unsat);
        }
        __syncthreads();
        if (ES && t > 1) {
            const uint32_t stopped = act & ~flag[t % 3];  // satisfied after iteration t - 1
            if (tid < BITS && (stopped >> tid & 1u)) its = t - 1;
            act &= ~stopped;
            if (tid == 0) flag[(t + 1) % 3] = 0u;  // last read before this barrier, next written after the next
            if (!act) break;
        }
        // ---- variable phase ----
        const bool last = !HASX && t == iters;
        for (int v = tid; v < n; v += T) {
            const int e0 = a.dv > 0 ? v * a.dv : a.vptr[v];
            const int d = a.dv > 0 ? a.dv : a.vptr[v + 1] - e0;
            const uint32_t y = Y[v];
            const uint32_t x = a.dv == 3 ? gb_variable<P, 3>(M, a.vslot, e0, 3, y, a.b)
                                         : gb_variable<P, 0>(M, a.vslot, e0, d, y, a.b);
            if constexpr (HASX) {
                const uint32_t old = X[v];
                const uint32_t nw = (old & ~act) | (x & act);
                X[v] = (P)nw;
                if constexpr (MC) {
                    uint32_t q = (old ^ nw) & FULL;
                    while (q) {
                        const int i = __builtin_ctz(q);
                        q &= q - 1u;
                        atomicAdd(&cnt[i], (nw >> i & 1u) ? 1 : -1);
                    }
                }
            } else if (last) {
                Y[v] = (P)x;  // nothing reads y again
            }
        }
        __syncthreads();
        if (MC && tid < nloc) a.trial[(size_t)(b0 + tid) * (iters + 1) + t] = cnt[tid];
    }
    // ---- results ----
    if (MC) {
        if (tid < nloc) {  // a workgroup that ended early: the tail repeats the stopping iteration's count
            int32_t *tr = a.trial + (size_t)(b0 + tid) * (iters + 1);
            const int c = cnt[tid];
            for (int j = t; j <= iters; ++j) tr[j] = c;
            a.its[b0 + tid] = its;
        }
        return;
    }
    if (a.its && tid < nloc) a.its[b0 + tid] = its;
    if (a.hard)
        for (int v = tid; v < n; v += T) {
            const uint32_t w = X[v];
            for (int i = 0; i < nloc; ++i) a.hard[(size_t)(b0 + i) * n + v] = (uint8_t)(w >> i & 1u);
        }
}

template <int T, typename P>
hipError_t launch_modes(const GbPlan &p, const GbArgs &a, bool es, bool mc, hipStream_t s) {
    const auto go = [&](auto kernel) { return launch_lds(kernel, dim3((unsigned)p.grid), dim3(T), p.lds, s, a); };
    if (mc) return es ? go(gb_kernel<T, P, true, true>) : go(gb_kernel<T, P, false, true>);
    return es ? go(gb_kernel<T, P, true, false>) : go(gb_kernel<T, P, false, false>);
}

// The instantiations: the rows of the shape table (kernel_shapes.hpp), from which gb_plan takes the
// shape it names.  The graph's tables and shape come from g.
hipError_t launch_gb(const GbPlan &p, const ldpc_graph &g, GbArgs a, bool es, bool mc, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    a.cptr = g.cptr, a.cvar = g.cvar, a.vptr = g.vptr, a.vslot = g.vslot;
    a.n = g.n, a.m = g.m, a.E = g.E, a.dv = g.dv, a.dc = g.dc;
#define LDPC_ROW(T, P, TAG) \
    if (p.threads == T && p.plane == (int)sizeof(P)) return launch_modes<T, P>(p, a, es, mc, s);
    LDPC_GB_SHAPES(LDPC_ROW)
#undef LDPC_ROW
    return hipErrorInvalidValue;  // a shape without a row: the plan gives none
}

}  // namespace

hipError_t launch_gb_decode(const GbPlan &p, const ldpc_graph &g, const uint8_t *d_bits, int B, int max_iters, int b,
                            bool early_stop, uint8_t *d_hard, int32_t *d_its, hipStream_t stream) {
    GbArgs a{};
    a.B = B, a.max_iters = max_iters, a.b = b;
    a.bits = d_bits, a.hard = d_hard, a.its = d_its;
    return launch_gb(p, g, a, early_stop, false, stream);
}

hipError_t launch_mc_gb(const GbPlan &p, const ldpc_graph &g, const ChanArgs &ch, uint64_t first_cw, int B,
                        int max_iters, int b, bool early_stop, int32_t *trial, int32_t *trial_its, hipStream_t stream) {
    GbArgs a{};
    a.B = B, a.max_iters = max_iters, a.b = b;
    a.ch = ch, a.first_cw = first_cw, a.trial = trial, a.its = trial_its;
    return launch_gb(p, g, a, early_stop, true, stream);
}

}  // namespace ldpc
