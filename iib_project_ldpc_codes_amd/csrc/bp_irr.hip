// bp_irr_kernel: irregular graphs on the host-built row layout, and its launch ladder.
#include "bp_device.hpp"

namespace ldpc {
namespace {

#ifndef LDPC_IRR_UV
#define LDPC_IRR_UV 1  // variables per load batch in bp_irr_kernel's variable phase (2, 4: no faster)
#endif
// ---------------------------------------------------------------------------
// 2b'. Irregular graphs (variable degree <= 4, check degree <= 8), one codeword
// per 1024-thread workgroup, host-built layout (build_irr_layout, graph_host.cpp):
//   check c = k*1024 + t is thread t's row-k check; its slot j sits at position
//   (k*DC + j)*1024 + t, so a row's reads and writes are lane-contiguous (LDS
//   conflict-free, coalesced in the slab).  Absent slots (degree < DC) hold the
//   rule's neutral input (min-sum +inf; sum-product skips them by degree) and are never
//   written, so the update runs on DC entries without a degree test (x1 and
//   min(+inf, .) change nothing: same values as oracle check_update_*(x, d)).
//   Positions [0, S) are in LDS, [S, P) in a per-workgroup global slab (whole
//   rows, so the row loop branches uniformly); the grid is one workgroup per CU
//   so the slabs stay L2-resident.
//   Lane p = i*1024 + t is thread t's i-th variable; lanes are sorted by degree
//   and each degree class is padded to whole 64-lane rows, so "edge j present"
//   is wave-uniform (readfirstlane).  Positions (2 x 16 bit per VGPR) and channel
//   LLRs stay in VGPRs for the whole decode; one variable's messages may sit in
//   LDS or in the slab (per-lane branch).
//   ET: the variable phase XORs the hard decision of every negative posterior
//   into a per-check syndrome bit array in LDS, tested after the phase.
// ---------------------------------------------------------------------------
template <int DC, int VPT, int ALGO, bool ET, bool MC>
__global__ __launch_bounds__(kIrrT) void bp_irr_kernel(BpArgs a) {
    constexpr int T = kIrrT;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int n = a.n, m = a.m, iters = a.max_iters, KC = a.irr_KC, S = a.irr_S;
    lds_f32 *ml = (lds_f32 *)(lds_u8 *)smem;  // [S]
    uint32_t *syn = reinterpret_cast<uint32_t *>(smem + (((size_t)S * 4 + 15) & ~(size_t)15));  // [m/32]
    const int nsyn = (m + 31) >> 5;
    int *curve = reinterpret_cast<int *>(syn + ((nsyn + 3) & ~3));  // [iters+1]
    float *slab = a.scratch + (size_t)blockIdx.x * a.irr_P;
    auto LD = [&](uint32_t q) -> float { return (int)q < S ? (float)ml[q] : slab[q]; };
    auto ST = [&](uint32_t q, float x) {
        if ((int)q < S) ml[q] = x;
        else slab[q] = x;
    };
    constexpr float neutral = ALGO == 0 ? 1.0f : __builtin_inff();
    const uint64_t cd = (uint32_t)a.irr_cdeg[tid] | ((uint64_t)(uint32_t)a.irr_cdeg[T + tid] << 32);
    uint32_t pp[2 * VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        pp[2 * i] = (uint32_t)a.irr_lane[(size_t)T * VPT + i * T + tid];
        pp[2 * i + 1] = (uint32_t)a.irr_lane[(size_t)2 * T * VPT + i * T + tid];
    }
    auto POS = [&](int i, int j) -> uint32_t {
        const uint32_t w = pp[2 * i + (j >> 1)];
        return (j & 1) ? (w >> 16) : (w & 0xFFFFu);
    };

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        __syncthreads();  // previous codeword drained (messages, curve, syndrome)
        if (MC) {
            for (int i = tid; i <= iters; i += T) curve[i] = 0;
        }
        // absent check slots -> neutral
        for (int k = 0; k < KC; ++k) {
            const int d = (int)((cd >> (4 * k)) & 15u);
            for (int j = d; j < DC; ++j) ST((uint32_t)((k * DC + j) * T + tid), neutral);
        }
        // channel LLRs and the first variable-to-check messages
        float L[VPT];
        int err0 = 0;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int v = a.irr_lane[i * T + tid];
            float l = 0.0f;
            if (v >= 0) l = MC ? chan_soft(a.ch, cw, v) : a.llr[(size_t)b * n + v];
            err0 += (v >= 0) & (l < 0.0f);
            L[i] = to_msg<ALGO>(l);
            const float w = v2c_rwire<ALGO>(L[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (__builtin_amdgcn_readfirstlane(POS(i, j)) != 0xFFFFu) ST(POS(i, j), w);
        }
        if (ET)
            for (int i = tid; i < nsyn; i += T) syn[i] = 0u;
        __syncthreads();
        if (MC) {
            const int w = wave_sum(err0);
            if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[0], w);
        }
        float pr[(ET && !MC) ? VPT : 1];
        if constexpr (ET && !MC) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) pr[i] = L[i];
        }
        // variable phase; FINAL = the last fixed-count iteration: outputs instead of messages
        auto var_phase = [&](auto final_tag) {
            constexpr bool FINAL = decltype(final_tag)::value;
            int errs = 0;
            // launder the packed positions: unpacked (and slab addresses) hoisted out
            // of the iteration loop would need ~4*VPT more VGPRs
#pragma unroll
            for (int q = 0; q < 2 * VPT; ++q) asm volatile("" : "+v"(pp[q]));
            // LDPC_IRR_UV variables per step: all their loads issue before the first
            // store (stores and later loads may alias as far as the compiler knows)
#pragma unroll
            for (int i0 = 0; i0 < VPT; i0 += LDPC_IRR_UV) {
                bool has[LDPC_IRR_UV][4];
                float cv[LDPC_IRR_UV][4];
#pragma unroll
                for (int u = 0; u < LDPC_IRR_UV; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = i0 + u;
                        has[u][j] = i < VPT && __builtin_amdgcn_readfirstlane(POS(i < VPT ? i : 0, j)) != 0xFFFFu;
                        cv[u][j] = has[u][j] ? LD(POS(i < VPT ? i : 0, j)) : 0.0f;
                    }
#pragma unroll
                for (int u = 0; u < LDPC_IRR_UV; ++u) {
                    const int i = i0 + u;
                    if (i >= VPT) break;
                    float s = L[i];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (has[u][j]) s += cv[u][j];
                    if constexpr (!FINAL) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (has[u][j]) ST(POS(i, j), v2c_rwire<ALGO>(s - cv[u][j]));
                    }
                    if constexpr (ET) {
                        if (s < 0.0f) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int q = (int)POS(i, j);
                                if (has[u][j] && q < KC * DC * T) {  // a check slot (not a dummy)
                                    const int c = (q / (DC * T)) * T + (q % T);
                                    atomicXor(&syn[c >> 5], 1u << (c & 31));
                                }
                            }
                        }
                        if constexpr (!MC) pr[i] = s;
                    }
                    if constexpr (MC) errs += (s < 0.0f);
                    if constexpr (FINAL && !MC) {
                        const int v = a.irr_lane[i * T + tid];
                        if (v >= 0) {
                            if (a.post) a.post[(size_t)b * n + v] = s * Domain<ALGO>::out;
                            if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(s < 0.0f);
                        }
                    }
                }
            }
            return errs;
        };

        int it = 0;
        for (; it < iters; ++it) {
            if (!ET && it > 0) __syncthreads();  // variable phase complete (ET: its syndrome barriers)
            // ---- check phase ----
            for (int k = 0; k < KC; ++k) {
                const int d = (int)((cd >> (4 * k)) & 15u);
                const int q0 = k * DC * T + tid;
                float x[DC];
                const bool in_lds = (k + 1) * DC * T <= S;  // uniform: whole rows
                if (in_lds) {
#pragma unroll
                    for (int j = 0; j < DC; ++j) x[j] = ml[q0 + j * T];
                } else {
#pragma unroll
                    for (int j = 0; j < DC; ++j) x[j] = slab[q0 + j * T];
                }
                if constexpr (ALGO == 1 && DC == 6) check_update_ms6(x, a.alpha);
                else check_update<ALGO, DC, true>(x, a.alpha, d);
                if (in_lds) {
#pragma unroll
                    for (int j = 0; j < DC; ++j)
                        if (j < d) ml[q0 + j * T] = x[j];
                } else {
#pragma unroll
                    for (int j = 0; j < DC; ++j)
                        if (j < d) slab[q0 + j * T] = x[j];
                }
            }
            __syncthreads();
            // fixed-count decode: the last variable phase runs after the loop
            if (!ET && !MC && it == iters - 1) break;
            const int errs = var_phase(std::false_type{});
            if (MC) {
                const int w = wave_sum(errs);
                if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[it + 1], w);
            }
            if constexpr (ET) {
                __syncthreads();  // syndrome complete
                int unsat = 0;
                for (int i = tid; i < nsyn; i += T) unsat |= (syn[i] != 0u);
                const bool more = __syncthreads_or(unsat);
                for (int i = tid; i < nsyn; i += T) syn[i] = 0u;  // every read is before that barrier
                if (!more) {
                    ++it;
                    break;
                }
            }
        }
        if (!ET && !MC && iters > 0) {
            (void)var_phase(std::true_type{});
            it = iters;
        }
        if constexpr (ET && !MC) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int v = a.irr_lane[i * T + tid];
                if (v >= 0) {
                    if (a.post) a.post[(size_t)b * n + v] = pr[i] * Domain<ALGO>::out;
                    if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(pr[i] < 0.0f);
                }
            }
        }
        if (!ET && !MC && iters == 0) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int v = a.irr_lane[i * T + tid];
                if (v >= 0) {
                    if (a.post) a.post[(size_t)b * n + v] = L[i] * Domain<ALGO>::out;
                    if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(L[i] < 0.0f);
                }
            }
        }
        if constexpr (MC) {
            __syncthreads();
            int32_t *tr = a.trial + (size_t)b * (iters + 1);
            const int last = curve[it];
            for (int i = tid; i <= iters; i += T) tr[i] = i <= it ? curve[i] : last;
            if (tid == 0) a.its[b] = it;
        } else {
            if (a.its && tid == 0) a.its[b] = it;
        }
    }
}

template <int DC, int VPT, int ALGO, bool ET, bool MC>
hipError_t launch_irr_shape(const BpPlan &p, const BpArgs &a, hipStream_t s) {
    return launch_lds(bp_irr_kernel<DC, VPT, ALGO, ET, MC>, dim3(p.grid), dim3(kIrrT), p.lds, s, a);
}

template <int ALGO, bool ET, bool MC>
hipError_t launch_irr_modes(const BpPlan &p, const ldpc_graph &g, BpArgs a, hipStream_t s) {
    a.irr_lane = g.irr_lane;
    a.irr_cdeg = g.irr_cdeg;
    a.irr_KC = g.irr_KC;
    a.irr_S = g.irr_S;
    a.irr_P = g.irr_P;
#define IRR_CASE(DC, VPT) \
    if (g.irr_DC == DC && g.irr_VPT == VPT) return launch_irr_shape<DC, VPT, ALGO, ET, MC>(p, a, s);
    // every VPT build_irr_layout hands out (1 and 2: graphs of up to 1024 / 2048 variable lanes)
    IRR_CASE(6, 1) IRR_CASE(6, 2) IRR_CASE(6, 5) IRR_CASE(6, 10) IRR_CASE(6, 20)
    IRR_CASE(8, 1) IRR_CASE(8, 2) IRR_CASE(8, 5) IRR_CASE(8, 10) IRR_CASE(8, 20)
#undef IRR_CASE
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_irr(const BpPlan &p, const ldpc_graph &g, BpArgs a, int algo, bool et, bool mc, hipStream_t s) {
    return bp_modes(algo, et, mc, [&](auto A, auto E, auto M) {
        return launch_irr_modes<decltype(A)::value, decltype(E)::value, decltype(M)::value>(p, g, a, s);
    });
}

}  // namespace ldpc
