// bp_ens_kernel: soft decoding over the random (dv, dc) ensemble -- codeword b on its own graph,
// rows b of the sampler's two lists -- and its launchers.
#include "bp_device.hpp"

namespace ldpc {
namespace {

// ---------------------------------------------------------------------------
// 2c. Ensemble path: one workgroup decodes one codeword on the regular graph the sampler
//   (sampler.hip) wrote for it: check_lookup[b][E] (slot c*dc + j -> variable) and
//   variable_lookup[b][E] (edge v*dv + i -> check, ascending); cptr / vptr are implicit.
//   No host-built layout exists for such a graph, so the workgroup builds the one index the
//   lists lack -- the slot of every variable edge inside its check -- once per codeword, before
//   iteration 0: slot s of check c = s / dc holds variable v, and the edge of v that names c is
//   found by a scan of v's dv entries (unambiguous: the sampler rejects a repeated variable in a
//   check).  The index lives in the workgroup's own block, never in a [B][E] table.
//   Block: messages float[E] | channel LLRs float[n] | cross index int32[E] (ens_block_bytes),
//   in LDS, or (GMEM) in a per-workgroup global slab with the first lds_slots messages in LDS.
//   Arithmetic and semantics are bp_generic_kernel's: the same check_update, variable sums from
//   the channel LLR in variable_lookup order, early stop on the syndrome of the previous
//   iteration's decisions, the same its / curve / tail fill.  The syndrome is kept as one bit per
//   check in LDS (ens_syn_bytes: two buffers, filled and read in alternate iterations): a
//   variable decided 1 flips the bits of its dv checks (slot / dc) with LDS atomics, so no
//   per-slot decision byte is scattered to the slab.  Both lists are only read.
// ---------------------------------------------------------------------------
constexpr int kEnsDV = 4;  // variable degrees up to this keep their messages in registers
#ifndef LDPC_ENS_UV
#define LDPC_ENS_UV 4  // variables per step of the variable phase (loads batched)
#endif

template <int T, int MAXDC, int ALGO, bool ET, bool MC, bool GMEM>
__global__ __launch_bounds__(T) void bp_ens_kernel(EnsArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    // checks per step of the check phase: two while a check's inputs are few registers
    constexpr int UC = MAXDC <= 8 ? 2 : 1;
    const int tid = threadIdx.x;
    const int n = a.n, m = a.m, E = a.E, dv = a.dv, dc = a.dc, iters = a.max_iters;
    const size_t block = ens_block_bytes((size_t)n, (size_t)E);
    unsigned char *base = GMEM ? reinterpret_cast<unsigned char *>(a.scratch) + (size_t)blockIdx.x * block : smem;
    float *msg_all = reinterpret_cast<float *>(base);
    float *Ls = msg_all + E;
    int32_t *xs = reinterpret_cast<int32_t *>(Ls + n);  // edge v*dv + i -> its slot
    // LDS beside the block: [block] syndrome bits, curve; GMEM: curve (16-byte padded), syndrome
    // bits, then the message slots
    const size_t curve_pad = MC ? (((size_t)(iters + 1) * 4 + 15) & ~(size_t)15) : 0;
    const int nsw = (m + 31) >> 5;  // words of one syndrome buffer
    unsigned int *syn = reinterpret_cast<unsigned int *>(GMEM ? smem + curve_pad : smem + block);
    int *curve = reinterpret_cast<int *>(GMEM ? smem : smem + block + ens_syn_bytes((size_t)m));
    // GMEM: the first S message slots live in LDS, the rest in the slab (explicit address
    // spaces, as bp_generic_kernel)
    const int S = GMEM ? a.lds_slots : 0;
    lds_f32 *msg_lds = (lds_f32 *)((lds_u8 *)smem + curve_pad + ens_syn_bytes((size_t)m));
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
        const int32_t *chk = a.chk + (size_t)b * E, *var = a.var + (size_t)b * E;
        __syncthreads();  // previous codeword fully drained
        if (MC) {
            for (int i = tid; i <= iters; i += T) curve[i] = 0;
        }
        int err0 = 0;
        for (int v = tid; v < n; v += T) {
            const float l = MC ? chan_soft(a.ch, cw, v) : a.llr[(size_t)b * n + v];
            Ls[v] = to_msg<ALGO>(l);
            err0 += (l < 0.0f);
            // a list that breaks the precondition leaves the edge on slot 0: wrong, but in bounds
            for (int i = 0; i < dv; ++i) xs[v * dv + i] = 0;
            if (!MC) {
                if (a.post) a.post[(size_t)b * n + v] = l;
                if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(l < 0.0f);
            }
        }
        __syncthreads();  // Ls, the cleared index and the zeroed curve
        if (MC) {
            const int w = wave_sum(err0);
            if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[0], w);
        }
        // slot-major: the list reads and the first messages are coalesced, the scan reads dv
        // neighbouring words of variable_lookup
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
        __syncthreads();
        int it = 0;
        for (; it < iters; ++it) {
            if (it > 0) __syncthreads();  // variable phase (messages, syndrome bits) complete
            int unsat = 0;                // ET: syndrome of the previous hard decisions
            unsigned int *syn_now = syn + (it & 1) * nsw;  // filled by this iteration's variable phase
            if (ET) {
                const unsigned int *syn_prev = syn + ((it & 1) ^ 1) * nsw;
                for (int w = tid; w < nsw; w += T) {
                    if (it > 0) unsat |= (syn_prev[w] != 0);
                    syn_now[w] = 0;  // last read one iteration ago
                }
            }
            for (int c0 = tid; c0 < m; c0 += T * UC) {
                int s0[UC], d[UC];
#pragma unroll
                for (int u = 0; u < UC; ++u) {
                    const int c = c0 + u * T;
                    s0[u] = (c < m ? c : m - 1) * dc;
                    d[u] = c < m ? dc : 0;
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
            if (dv <= kEnsDV) {  // slots and messages read once, kept in registers
                for (int v0 = tid; v0 < n; v0 += T * LDPC_ENS_UV) {
                    int sl[LDPC_ENS_UV][kEnsDV];
                    float cv[LDPC_ENS_UV][kEnsDV], sv[LDPC_ENS_UV];
#pragma unroll
                    for (int u = 0; u < LDPC_ENS_UV; ++u) {
                        const int v = v0 + u * T, vc = v < n ? v : n - 1;  // clamped: loads stay unconditional
                        sv[u] = Ls[vc];
#pragma unroll
                        for (int j = 0; j < kEnsDV; ++j) sl[u][j] = j < dv ? xs[vc * dv + j] : 0;
                    }
#pragma unroll
                    for (int u = 0; u < LDPC_ENS_UV; ++u)
#pragma unroll
                        for (int j = 0; j < kEnsDV; ++j) cv[u][j] = j < dv ? LD(sl[u][j]) : 0.0f;
#pragma unroll
                    for (int u = 0; u < LDPC_ENS_UV; ++u) {
                        const int v = v0 + u * T;
                        if (v >= n) continue;
                        float s = sv[u];
#pragma unroll
                        for (int j = 0; j < kEnsDV; ++j) s += cv[u][j];  // absent edges add +0
#pragma unroll
                        for (int j = 0; j < kEnsDV; ++j)
                            if (j < dv) ST(sl[u][j], s - cv[u][j]);
                        if (ET && s < 0.0f) {
                            for (int j = 0; j < kEnsDV; ++j)
                                if (j < dv) {
                                    const int c = sl[u][j] / dc;
                                    atomicXor(&syn_now[c >> 5], 1u << (c & 31));
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
hipError_t launch_ens_shape(const BpPlan &p, EnsArgs a, hipStream_t s) {
    constexpr int T = GMEM ? LDPC_GMEM_T : 256;
    auto k = bp_ens_kernel<T, MAXDC, ALGO, ET, MC, GMEM>;
    a.lds_slots = p.lds_slots;
    hipError_t e = allow_lds(k, p.lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(p.grid), dim3(T), p.lds, s, a);
    return hipGetLastError();
}

template <int ALGO, bool ET, bool MC>
hipError_t launch_ens_modes(const BpPlan &p, const EnsArgs &a, hipStream_t s) {
    switch (p.path) {
        case BpPath::Ens8: return launch_ens_shape<8, ALGO, ET, MC, false>(p, a, s);
        case BpPath::Ens16: return launch_ens_shape<16, ALGO, ET, MC, false>(p, a, s);
        case BpPath::Ens32: return launch_ens_shape<32, ALGO, ET, MC, false>(p, a, s);
        case BpPath::EnsG8: return launch_ens_shape<8, ALGO, ET, MC, true>(p, a, s);
        case BpPath::EnsG16: return launch_ens_shape<16, ALGO, ET, MC, true>(p, a, s);
        case BpPath::EnsG32: return launch_ens_shape<32, ALGO, ET, MC, true>(p, a, s);
        default: return hipErrorNotSupported;
    }
}

EnsArgs ens_args(int n, int dv, int dc, const int32_t *chk, const int32_t *var, int B, int iters, float alpha) {
    EnsArgs a{};
    a.chk = chk;
    a.var = var;
    a.n = n;
    a.dv = dv;
    a.dc = dc;
    a.E = n * dv;
    a.m = a.E / dc;
    a.B = B;
    a.max_iters = iters;
    a.alpha = alpha;
    return a;
}

hipError_t launch_ens(EnsArgs a, float *d_scratch, size_t scratch_bytes, int algo, bool et, bool mc, hipStream_t s) {
    const BpPlan p = bp_ens_plan(a.n, a.dv, a.dc, a.B, a.max_iters, algo, et, mc, a.post != nullptr, device_cus());
    if (p.path == BpPath::None) return hipErrorNotSupported;
    // a caller that sized the buffer by another rule than bp_ens_plan's fails loudly
    if (p.scratch > (d_scratch ? scratch_bytes : 0)) return hipErrorInvalidValue;
    a.scratch = d_scratch;
    return bp_modes(algo, et, mc, [&](auto A, auto E, auto M) {
        return launch_ens_modes<decltype(A)::value, decltype(E)::value, decltype(M)::value>(p, a, s);
    });
}

}  // namespace

size_t ens_scratch_bytes(int n, int dv, int dc, int B, int iters, int algo, bool early_stop, bool mc, bool want_post) {
    return bp_ens_plan(n, dv, dc, B, iters, algo, early_stop, mc, want_post, device_cus()).scratch;
}

hipError_t launch_ens_decode(int n, int dv, int dc, const int32_t *check_lookup, const int32_t *variable_lookup,
                             const float *d_llr, int B, int max_iters, int algo, float alpha, int early_stop,
                             float *d_post, uint8_t *d_hard, int32_t *d_its, hipStream_t stream, float *d_scratch,
                             size_t scratch_bytes) {
    if (B <= 0) return hipSuccess;
    EnsArgs a = ens_args(n, dv, dc, check_lookup, variable_lookup, B, max_iters, alpha);
    a.llr = d_llr;
    a.post = d_post;
    a.hard = d_hard;
    a.its = d_its;
    return launch_ens(a, d_scratch, scratch_bytes, algo, early_stop != 0, false, stream);
}

hipError_t launch_mc_ens(int n, int dv, int dc, const int32_t *check_lookup, const int32_t *variable_lookup,
                         int channel, float p, float p2, uint64_t seed, uint64_t first_cw, int B, int max_iters,
                         int algo, float alpha, int early_stop, int32_t *trial, int32_t *trial_its,
                         hipStream_t stream, float *d_scratch, size_t scratch_bytes) {
    if (B <= 0) return hipSuccess;
    EnsArgs a = ens_args(n, dv, dc, check_lookup, variable_lookup, B, max_iters, alpha);
    a.ch = make_chan(channel, p, p2, seed);
    a.first_cw = first_cw;
    a.trial = trial;
    a.its = trial_its;
    return launch_ens(a, d_scratch, scratch_bytes, algo, early_stop != 0, true, stream);
}

}  // namespace ldpc
