// The flooding decode loop of bp_generic_kernel (bp_generic.hip) and bp_ens_kernel (bp_ens.hip),
// and their launch ladder.  One workgroup decodes one codeword at a time on a block
//   messages float[E] (check-major slots) | channel LLRs float[n] | the graph view's index
// in LDS, or (GMEM) in a per-workgroup global slab (it stays L2 / Infinity-Cache resident) with
// the first lds_slots messages in LDS.  Posterior / hard decision are written to the outputs
// after a variable phase.  Two graph views, chosen by the argument struct:
//   CSR (BpArgs): check spans from cptr, variable edges and slots from vptr / vslot, the
//     register path chosen per variable; index = decision bytes u8[E] (generic_block_bytes), the
//     early-stop syndrome is the decision of every slot's variable, XORed over a check's slots
//     in the next check phase.
//   Ensemble (EnsArgs): word b on rows b of the sampler's check_lookup / variable_lookup, spans
//     implicit (c dc, v dv), the register path chosen per workgroup; index = the slot of every
//     variable edge, int32[E] (ens_block_bytes), built per codeword before iteration 0; the
//     syndrome is one bit per check in LDS (ens_syn_bytes), see bp_ens.hip.
//
// Each of the two files includes this once, after defining LDPC_FLOOD_KERNEL (the kernel's name)
// and LDPC_FLOOD_ARGS (its argument struct).  The loop and what differs between the views
// (`if constexpr (ENS)`) are the text of the __global__ function itself, not device functions it
// calls: a function is optimised once on its own and again after inlining, and the kernels then
// allocate other registers than the same text written in place (the whole body as a function:
// sum-product <16,lds> 99 VGPRs against 88; the views' syndrome hooks as functions: 1-2 VGPRs
// more in every early-stop decode kernel).  For the same reason the looped variable path and the
// decision outputs stand once per view and not in a shared lambda.
#include <type_traits>

#include "bp_device.hpp"

#ifndef LDPC_GEN_UC
#define LDPC_GEN_UC 2  // checks per step of the generic kernel's check phase (loads batched)
#endif
#ifndef LDPC_GEN_UV
#define LDPC_GEN_UV 4  // variables per step of the generic kernel's variable phase
#endif
#ifndef LDPC_ENS_UV
#define LDPC_ENS_UV 4  // variables per step of the ensemble kernel's variable phase
#endif

namespace ldpc {
namespace {

constexpr int kFloodDV = 4;  // variable degrees up to this keep their messages in registers

template <int T, int MAXDC, int ALGO, bool ET, bool MC, bool GMEM>
__global__ __launch_bounds__(T) void LDPC_FLOOD_KERNEL(LDPC_FLOOD_ARGS a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr bool ENS = std::is_same<LDPC_FLOOD_ARGS, EnsArgs>::value;
    // checks / variables per step: every load of a step is issued before the first use, so the
    // L2 latency of the index and slab reads overlaps.  Ensemble: two checks while a check's
    // inputs are few registers
    constexpr int UC = ENS ? (MAXDC <= 8 ? 2 : 1) : LDPC_GEN_UC, UV = ENS ? LDPC_ENS_UV : LDPC_GEN_UV;
    // the arguments as a type-dependent expression, so that a discarded `if constexpr` branch may
    // name the other view's fields
    const auto &g = static_cast<const std::conditional_t<(T > 0), LDPC_FLOOD_ARGS, void> &>(a);
    const int tid = threadIdx.x;
    const int n = a.n, m = a.m, E = a.E, iters = a.max_iters;
    int dv = 0, dc = 0;
    if constexpr (ENS) dv = g.dv, dc = g.dc;
    const size_t block = ENS ? ens_block_bytes((size_t)n, (size_t)E) : generic_block_bytes((size_t)n, (size_t)E);
    unsigned char *base = GMEM ? reinterpret_cast<unsigned char *>(a.scratch) + (size_t)blockIdx.x * block : smem;
    float *msg_all = reinterpret_cast<float *>(base);
    float *Ls = msg_all + E;
    uint8_t *hs = reinterpret_cast<uint8_t *>(Ls + n);  // CSR: slot -> last decision of its variable
    int32_t *xs = reinterpret_cast<int32_t *>(Ls + n);  // ensemble: edge v*dv + i -> its slot
    // LDS beside the block: [block] syndrome bits, curve; GMEM: curve (16-byte padded), syndrome
    // bits, then the message slots
    const size_t curve_pad = MC ? curve_bytes(iters) : 0;
    const int nsw = (m + 31) >> 5;  // words of one syndrome buffer
    unsigned int *syn = reinterpret_cast<unsigned int *>(GMEM ? smem + curve_pad : smem + block);
    const size_t syn_bytes = ENS ? ens_syn_bytes((size_t)m) : 0;
    int *curve = reinterpret_cast<int *>(GMEM ? smem : smem + block + syn_bytes);
    // GMEM: the first S message slots live in LDS, the rest in the slab
    const int S = GMEM ? a.lds_slots : 0;
    // explicit address spaces (no generic pointer selects: a select between an LDS
    // and a global pointer trips the gfx950 backend once the loops are unrolled)
    lds_f32 *msg_lds = (lds_f32 *)((lds_u8 *)smem + curve_pad + syn_bytes);
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
    // Monte-Carlo: bit errors of the workgroup's decisions into curve[i]
    auto count = [&](int i, int errs) {
        if (MC) {
            const int w = wave_sum(errs);
            if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[i], w);
        }
    };

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        const int32_t *chk = nullptr, *var = nullptr;
        if constexpr (ENS) chk = g.chk + (size_t)b * E, var = g.var + (size_t)b * E;
        __syncthreads();  // previous codeword fully drained
        if (MC) {
            for (int i = tid; i <= iters; i += T) curve[i] = 0;
        }
        if constexpr (!ENS) __syncthreads();  // ensemble: fenced after the loop below
        int err0 = 0;
        for (int v = tid; v < n; v += T) {
            const float l = MC ? chan_soft(a.ch, cw, v) : a.llr[(size_t)b * n + v];
            const float l2 = to_msg<ALGO>(l);
            Ls[v] = l2;
            err0 += (l < 0.0f);
            if constexpr (ENS) {
                // a list that breaks the precondition leaves the edge on slot 0: wrong, but in bounds
                for (int i = 0; i < dv; ++i) xs[v * dv + i] = 0;
            } else {
                for (int e = g.vptr[v]; e < g.vptr[v + 1]; ++e) ST(g.vslot[e], l2);
            }
            if (!MC) {
                if (a.post) a.post[(size_t)b * n + v] = l;
                if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(l < 0.0f);
            }
        }
        if constexpr (ENS) __syncthreads();  // Ls, the cleared index and the zeroed curve
        count(0, err0);
        if constexpr (ENS) {
            // The index the lists lack, slot-major: the list reads and the first messages are
            // coalesced, the scan reads dv neighbouring words of variable_lookup
            for (int s = tid; s < E; s += T) {
                const int v = chk[s], c = s / dc;
                if ((unsigned)v >= (unsigned)n) {  // outside the precondition: keep every access in bounds
                    ST(s, 0.0f);
                    continue;
                }
                ST(s, Ls[v]);
                const int e0 = v * dv;
                for (int i = 0; i < dv; ++i)
                    if (var[e0 + i] == c) xs[e0 + i] = s;
            }
        }
        __syncthreads();
        int it = 0;
        for (; it < iters; ++it) {
            if (it > 0) __syncthreads();  // variable phase (messages, syndrome) complete
            int unsat = 0;                // ET: syndrome of the previous hard decisions
            unsigned int *syn_now = syn + (it & 1) * nsw;  // ensemble: filled by this iteration's variable phase
            if constexpr (ENS) {
                if (ET) {
                    const unsigned int *syn_prev = syn + ((it & 1) ^ 1) * nsw;
                    for (int w = tid; w < nsw; w += T) {
                        if (it > 0) unsat |= (syn_prev[w] != 0);
                        syn_now[w] = 0;  // last read one iteration ago
                    }
                }
            }
            for (int c0 = tid; c0 < m; c0 += T * UC) {
                int s0[UC], d[UC];
#pragma unroll
                for (int u = 0; u < UC; ++u) {
                    const int c = c0 + u * T, cc = c < m ? c : m - 1;  // clamped: the loads stay in bounds
                    if constexpr (ENS) {
                        s0[u] = cc * dc;
                        d[u] = c < m ? dc : 0;
                    } else {
                        s0[u] = g.cptr[cc];
                        d[u] = c < m ? g.cptr[cc + 1] - s0[u] : 0;
                    }
                }
                if constexpr (!ENS) {
                    if (ET && it > 0) {
#pragma unroll
                        for (int u = 0; u < UC; ++u) {
                            int par = 0;
                            for (int q = 0; q < d[u]; ++q) par ^= hs[s0[u] + q];
                            unsat |= par;
                        }
                    }
                }
                float x[UC][MAXDC];
#pragma unroll
                for (int u = 0; u < UC; ++u)
#pragma unroll
                    for (int q = 0; q < MAXDC; ++q) x[u][q] = q < d[u] ? LD(s0[u] + q) : __builtin_inff();
#pragma unroll
                for (int u = 0; u < UC; ++u) {
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
            // CSR: the register path is chosen per variable; ensemble: per workgroup
            if (!ENS || dv <= kFloodDV) {
                for (int v0 = tid; v0 < n; v0 += T * UV) {
                    int e0[UV], dg[UV], sl[UV][kFloodDV];
                    float sv[UV], cv[UV][kFloodDV];
#pragma unroll
                    for (int u = 0; u < UV; ++u) {
                        const int v = v0 + u * T, vc = v < n ? v : n - 1;  // clamped: loads stay unconditional
                        if constexpr (!ENS) {
                            e0[u] = g.vptr[vc];
                            dg[u] = v < n ? g.vptr[vc + 1] - e0[u] : 0;
                        }
                        sv[u] = Ls[vc];
                        if constexpr (ENS) {
                            e0[u] = vc * dv;
                            dg[u] = dv;
#pragma unroll
                            for (int j = 0; j < kFloodDV; ++j) sl[u][j] = j < dv ? xs[e0[u] + j] : 0;
                        }
                    }
                    if constexpr (!ENS) {
#pragma unroll
                        for (int u = 0; u < UV; ++u)
#pragma unroll
                            for (int j = 0; j < kFloodDV; ++j) sl[u][j] = j < dg[u] ? g.vslot[e0[u] + j] : 0;
                    }
#pragma unroll
                    for (int u = 0; u < UV; ++u)
#pragma unroll
                        for (int j = 0; j < kFloodDV; ++j) cv[u][j] = j < dg[u] ? LD(sl[u][j]) : 0.0f;
#pragma unroll
                    for (int u = 0; u < UV; ++u) {
                        const int v = v0 + u * T;
                        if (v >= n) continue;
                        float s = sv[u];
                        if (ENS || dg[u] <= kFloodDV) {  // messages and slots read once, kept in registers
#pragma unroll
                            for (int j = 0; j < kFloodDV; ++j) s += cv[u][j];  // absent edges add +0
#pragma unroll
                            for (int j = 0; j < kFloodDV; ++j)
                                if (j < dg[u]) {
                                    ST(sl[u][j], s - cv[u][j]);
                                    if constexpr (!ENS) {
                                        if (ET) hs[sl[u][j]] = (uint8_t)(s < 0.0f);
                                    }
                                }
                            if constexpr (ENS) {
                                if (ET && s < 0.0f) {
                                    for (int j = 0; j < kFloodDV; ++j)
                                        if (j < dv) {  // flip the syndrome bit of the slot's check
                                            const int c = sl[u][j] / dc;
                                            atomicXor(&syn_now[c >> 5], 1u << (c & 31));
                                        }
                                }
                            }
                        } else if constexpr (!ENS) {  // any degree: messages and slots read twice
                            const int e1 = e0[u] + dg[u];
                            for (int e = e0[u]; e < e1; ++e) s += LD(g.vslot[e]);
                            for (int e = e0[u]; e < e1; ++e) {
                                const int slot = g.vslot[e];
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
            } else {
                for (int v = tid; v < n; v += T) {
                    const int e0 = v * dv, e1 = e0 + dv;
                    float s = Ls[v];
                    for (int e = e0; e < e1; ++e) s += LD(xs[e]);
                    for (int e = e0; e < e1; ++e) {
                        const int slot = xs[e];
                        ST(slot, s - LD(slot));
                        if (ET && s < 0.0f) atomicXor(&syn_now[(slot / dc) >> 5], 1u << ((slot / dc) & 31));
                    }
                    errs += (s < 0.0f);
                    if (out_now) {
                        if (a.post) a.post[(size_t)b * n + v] = s * Domain<ALGO>::out;
                        if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(s < 0.0f);
                    }
                }
            }
            count(it + 1, errs);
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

// The launch ladder: `first` is the path of <8,lds>; <16,lds>, <32,lds>, <8,gmem>, <16,gmem>,
// <32,gmem> follow it in BpPath.  Any other path: no_kernel.
template <int MAXDC, int ALGO, bool ET, bool MC, bool GMEM>
hipError_t launch_flood_shape(const BpPlan &p, LDPC_FLOOD_ARGS a, hipStream_t s) {
    constexpr int T = GMEM ? LDPC_GMEM_T : 256;
    auto k = LDPC_FLOOD_KERNEL<T, MAXDC, ALGO, ET, MC, GMEM>;
    a.lds_slots = p.lds_slots;
    return launch_lds(k, dim3(p.grid), dim3(T), p.lds, s, a);
}

hipError_t launch_flood(const BpPlan &p, const LDPC_FLOOD_ARGS &a, int algo, bool et, bool mc, hipStream_t s,
                        BpPath first, hipError_t no_kernel) {
    return bp_modes(algo, et, mc, [&](auto A, auto E, auto M) {
        constexpr int ALGO = decltype(A)::value;
        constexpr bool ET = decltype(E)::value, MC = decltype(M)::value;
        switch ((int)p.path - (int)first) {
            case 0: return launch_flood_shape<8, ALGO, ET, MC, false>(p, a, s);
            case 1: return launch_flood_shape<16, ALGO, ET, MC, false>(p, a, s);
            case 2: return launch_flood_shape<32, ALGO, ET, MC, false>(p, a, s);
            case 3: return launch_flood_shape<8, ALGO, ET, MC, true>(p, a, s);
            case 4: return launch_flood_shape<16, ALGO, ET, MC, true>(p, a, s);
            case 5: return launch_flood_shape<32, ALGO, ET, MC, true>(p, a, s);
            default: return no_kernel;
        }
    });
}

}  // namespace
}  // namespace ldpc
