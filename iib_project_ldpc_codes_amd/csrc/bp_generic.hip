// bp_generic_kernel: any CSR graph with check degree <= 32, messages in LDS or in a
// per-workgroup global slab, and its launch ladder.
#include "bp_device.hpp"

namespace ldpc {
namespace {

// ---------------------------------------------------------------------------
// 2b. Generic path: any (irregular) CSR graph, check degree <= MAXDC.
//   Messages in LDS when they fit, else in a per-workgroup global scratch
//   slab (GMEM; the slab stays L2 / Infinity-Cache resident).  Channel LLRs
//   are kept beside the messages.  Posterior / hard decision are written to
//   the outputs after every variable phase.
// ---------------------------------------------------------------------------
constexpr int kGenDV = 4;  // variable degrees up to this keep their messages in registers
#ifndef LDPC_GEN_UC
#define LDPC_GEN_UC 2  // checks per step of the generic kernel's check phase (loads batched)
#endif
#ifndef LDPC_GEN_UV
#define LDPC_GEN_UV 4  // variables per step of the generic kernel's variable phase
#endif

template <int T, int MAXDC, int ALGO, bool ET, bool MC, bool GMEM>
__global__ __launch_bounds__(T) void bp_generic_kernel(BpArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int n = a.n, m = a.m, E = a.E, iters = a.max_iters;
    unsigned char *base = GMEM ? reinterpret_cast<unsigned char *>(a.scratch) +
                                     (size_t)blockIdx.x * (((size_t)E * 5 + (size_t)n * 4 + 15) & ~(size_t)15)
                               : smem;
    float *msg_all = reinterpret_cast<float *>(base);
    float *Ls = msg_all + E;
    uint8_t *hs = reinterpret_cast<uint8_t *>(Ls + n);
    int *curve = reinterpret_cast<int *>(GMEM ? smem : smem + (((size_t)E * 5 + (size_t)n * 4 + 15) & ~(size_t)15));
    // GMEM: the first S message slots live in LDS, the rest in the L2-resident
    // global slab (generic pointers -> flat loads pick the space per lane).
    const int S = GMEM ? a.lds_slots : 0;
    // explicit address spaces (no generic pointer selects: a select between an LDS
    // and a global pointer trips the gfx950 backend once the loops are unrolled)
    lds_f32 *msg_lds = (lds_f32 *)((lds_u8 *)smem + (MC ? (((size_t)(iters + 1) * 4 + 15) & ~(size_t)15) : 0));
    lds_f32 *msg_l = (lds_f32 *)(lds_u8 *)smem;  // !GMEM: every message in LDS
    auto LD = [&](int e) -> float {
        if constexpr (GMEM) return e < S ? msg_lds[e] : msg_all[e];
        else return msg_l[e];
    };
    auto ST = [&](int e, float x) {
        if constexpr (GMEM) {
            if (e < S) msg_lds[e] = x;
            else msg_all[e] = x;
        } else {
            msg_l[e] = x;
        }
    };

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        __syncthreads();  // previous codeword fully drained
        if (MC) {
            for (int i = tid; i <= iters; i += T) curve[i] = 0;
        }
        __syncthreads();
        int err0 = 0;
        for (int v = tid; v < n; v += T) {
            const float l = MC ? chan_soft(a.ch, cw, v) : a.llr[(size_t)b * n + v];
            const float l2 = to_msg<ALGO>(l);
            Ls[v] = l2;
            err0 += (l < 0.0f);
            for (int e = a.vptr[v]; e < a.vptr[v + 1]; ++e) ST(a.vslot[e], l2);
            if (!MC) {
                if (a.post) a.post[(size_t)b * n + v] = l;
                if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(l < 0.0f);
            }
        }
        if (MC) {
            const int w = wave_sum(err0);
            if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[0], w);
        }
        __syncthreads();
        int it = 0;
        for (; it < iters; ++it) {
            if (it > 0) __syncthreads();  // variable phase (messages, hs) complete
            int unsat = 0;                // ET: syndrome of the previous hard decisions
            // LDPC_GEN_UC checks per step: every load of the step is issued before
            // the first use, so the L2 latency of the CSR and slab reads overlaps
            for (int c0 = tid; c0 < m; c0 += T * LDPC_GEN_UC) {
                int s0[LDPC_GEN_UC], d[LDPC_GEN_UC];
#pragma unroll
                for (int u = 0; u < LDPC_GEN_UC; ++u) {
                    const int c = c0 + u * T, cc = c < m ? c : m - 1;
                    s0[u] = a.cptr[cc];
                    d[u] = c < m ? a.cptr[cc + 1] - s0[u] : 0;
                }
                if (ET && it > 0) {
#pragma unroll
                    for (int u = 0; u < LDPC_GEN_UC; ++u) {
                        int par = 0;
                        for (int q = 0; q < d[u]; ++q) par ^= hs[s0[u] + q];
                        unsat |= par;
                    }
                }
                float x[LDPC_GEN_UC][MAXDC];
#pragma unroll
                for (int u = 0; u < LDPC_GEN_UC; ++u)
#pragma unroll
                    for (int q = 0; q < MAXDC; ++q) x[u][q] = q < d[u] ? LD(s0[u] + q) : __builtin_inff();
#pragma unroll
                for (int u = 0; u < LDPC_GEN_UC; ++u) {
                    check_update<ALGO, MAXDC>(x[u], a.alpha, d[u]);
#pragma unroll
                    for (int q = 0; q < MAXDC; ++q)
                        if (q < d[u]) ST(s0[u] + q, x[u][q]);
                }
            }
            if constexpr (ET) {
                if (!__syncthreads_or(unsat | (it == 0))) break;
            } else {
                __syncthreads();
            }
            int errs = 0;
            // decisions leave the kernel only when they can be final: the last
            // fixed-count iteration, or every iteration under early stop
            const bool out_now = !MC && (ET || it == iters - 1);
            // LDPC_GEN_UV variables per step, loads batched as in the check phase
            for (int v0 = tid; v0 < n; v0 += T * LDPC_GEN_UV) {
                int e0[LDPC_GEN_UV], dg[LDPC_GEN_UV];
                float sv[LDPC_GEN_UV];
#pragma unroll
                for (int u = 0; u < LDPC_GEN_UV; ++u) {
                    const int v = v0 + u * T, vc = v < n ? v : n - 1;  // clamped: loads stay unconditional
                    e0[u] = a.vptr[vc];
                    dg[u] = v < n ? a.vptr[vc + 1] - e0[u] : 0;
                    sv[u] = Ls[vc];
                }
                int sl[LDPC_GEN_UV][kGenDV];
                float cv[LDPC_GEN_UV][kGenDV];
#pragma unroll
                for (int u = 0; u < LDPC_GEN_UV; ++u)
#pragma unroll
                    for (int j = 0; j < kGenDV; ++j) sl[u][j] = j < dg[u] ? a.vslot[e0[u] + j] : 0;
#pragma unroll
                for (int u = 0; u < LDPC_GEN_UV; ++u)
#pragma unroll
                    for (int j = 0; j < kGenDV; ++j) cv[u][j] = j < dg[u] ? LD(sl[u][j]) : 0.0f;
#pragma unroll
                for (int u = 0; u < LDPC_GEN_UV; ++u) {
                    const int v = v0 + u * T;
                    if (v >= n) continue;
                    float s = sv[u];
                    if (dg[u] <= kGenDV) {  // messages and slots read once, kept in registers
#pragma unroll
                        for (int j = 0; j < kGenDV; ++j) s += cv[u][j];  // absent edges add +0
#pragma unroll
                        for (int j = 0; j < kGenDV; ++j)
                            if (j < dg[u]) {
                                ST(sl[u][j], s - cv[u][j]);
                                if (ET) hs[sl[u][j]] = (uint8_t)(s < 0.0f);
                            }
                    } else {
                        const int e1 = e0[u] + dg[u];
                        for (int e = e0[u]; e < e1; ++e) s += LD(a.vslot[e]);
                        for (int e = e0[u]; e < e1; ++e) {
                            const int slot = a.vslot[e];
                            ST(slot, s - LD(slot));
                            if (ET) hs[slot] = (uint8_t)(s < 0.0f);
                        }
                    }
                    errs += (s < 0.0f);
                    if (out_now) {
                        if (a.post) a.post[(size_t)b * n + v] = s * Domain<ALGO>::out;
                        if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(s < 0.0f);
                    }
                }
            }
            if (MC) {
                const int w = wave_sum(errs);
                if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[it + 1], w);
            }
        }
        __syncthreads();
        if (MC) {
            int32_t *tr = a.trial + (size_t)b * (iters + 1);
            const int last = curve[it];
            for (int i = tid; i <= iters; i += T) tr[i] = i <= it ? curve[i] : last;
        }
        if ((MC || a.its) && tid == 0) a.its[b] = it;
    }
}

template <int MAXDC, int ALGO, bool ET, bool MC, bool GMEM>
hipError_t launch_generic_shape(const BpPlan &p, BpArgs a, hipStream_t s) {
    constexpr int T = GMEM ? LDPC_GMEM_T : 256;
    auto k = bp_generic_kernel<T, MAXDC, ALGO, ET, MC, GMEM>;
    a.lds_slots = p.lds_slots;
    hipError_t e = allow_lds(k, p.lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(p.grid), dim3(T), p.lds, s, a);
    return hipGetLastError();
}

template <int ALGO, bool ET, bool MC>
hipError_t launch_generic_modes(const BpPlan &p, const BpArgs &a, hipStream_t s) {
    switch (p.path) {
        case BpPath::Generic8: return launch_generic_shape<8, ALGO, ET, MC, false>(p, a, s);
        case BpPath::Generic16: return launch_generic_shape<16, ALGO, ET, MC, false>(p, a, s);
        case BpPath::Generic32: return launch_generic_shape<32, ALGO, ET, MC, false>(p, a, s);
        case BpPath::GenericG8: return launch_generic_shape<8, ALGO, ET, MC, true>(p, a, s);
        case BpPath::GenericG16: return launch_generic_shape<16, ALGO, ET, MC, true>(p, a, s);
        case BpPath::GenericG32: return launch_generic_shape<32, ALGO, ET, MC, true>(p, a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_generic(const BpPlan &p, const ldpc_graph &, BpArgs a, int algo, bool et, bool mc, hipStream_t s) {
    return bp_modes(algo, et, mc, [&](auto A, auto E, auto M) {
        return launch_generic_modes<decltype(A)::value, decltype(E)::value, decltype(M)::value>(p, a, s);
    });
}

}  // namespace ldpc
