// bp_layer_kernel: the layered (row-serial, "turbo-decoding message passing") schedule on a fixed
// code, for any graph with a layer schedule (check degree <= 32; build_layer_schedule,
// graph_host.cpp), and its launch ladder.  Semantics: include/ldpc_mi355x.h,
// ldpc_bp_layered_decode_batch_dev.
//
// One workgroup decodes one codeword at a time on a block
//   posteriors P float[n] | check->variable messages R float[E]
// in LDS, or (GMEM) in a per-workgroup global slab with the block's first lds_slots words -- P
// first: a posterior is touched once per edge of its variable, a message once -- in LDS.  The
// checks of a layer share no variable, so a layer is one parallel step: thread i takes
// positions i, i + T, ... of the layer, gathers its check's posteriors, subtracts the check's
// old messages, runs the flooding kernels' check rule (check_update, bp_device.hpp) and writes
// the new messages and posteriors back; one workgroup barrier ends the layer.  R lives at the
// index of its edge in lay_var (layer-ordered, lane-major: word lay_tab[l][j] + p is edge j of
// the check at position p of layer l), so the threads of a wave read neighbouring words of both.
// Sum-product works in the log2 domain (Domain<0>) as everywhere else.
#include "bp_device.hpp"

#ifndef LDPC_LAYER_UC
#define LDPC_LAYER_UC 2  // checks per step of a thread at check degrees <= 16 (loads batched)
#endif

namespace ldpc {
namespace {

template <int T, int MAXDC, int ALGO, bool ET, bool MC, bool GMEM>
__global__ __launch_bounds__(T) void bp_layer_kernel(LayerArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    // every load of a step is issued before the first use, as in bp_flood.hpp
    constexpr int UC = MAXDC <= 16 ? LDPC_LAYER_UC : 1;
    const int tid = threadIdx.x;
    const int n = a.n, E = a.E, iters = a.max_iters, L = a.L;
    // LDS: curve (16-byte padded, Monte-Carlo only) | the block's first S words
    const size_t curve_pad = MC ? curve_bytes(iters) : 0;
    int *curve = reinterpret_cast<int *>(smem);
    const int S = GMEM ? a.lds_slots : n + E;
    // explicit address spaces, as in bp_flood.hpp
    lds_f32 *blk_l = (lds_f32 *)((lds_u8 *)smem + curve_pad);
    float *blk_g = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(a.scratch) +
                                             (GMEM ? (size_t)blockIdx.x * layer_block_bytes((size_t)n, (size_t)E) : 0));
    auto LD = [&](int w) -> float {
        if constexpr (GMEM) return w < S ? blk_l[w] : blk_g[w];
        else return blk_l[w];
    };
    auto ST = [&](int w, float x) {
        if constexpr (GMEM) {
            if (w < S) blk_l[w] = x;
            else blk_g[w] = x;
        } else {
            blk_l[w] = x;
        }
    };
    // Monte-Carlo: bit errors of the workgroup's decisions into curve[i]
    auto count = [&](int i, int errs) {
        if (MC) {
            const int w = wave_sum(errs);
            if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[i], w);
        }
    };

    // Variables (and with them the degree) of the checks at positions p0 + u T of a layer: position
    // p has a j-th edge exactly when p is below the layer's count of them (lay_tab's row; past
    // the layer's last check none), so the loads depend on no other load.
    auto load_vars = [&](const int32_t *row, int p0, int (&d)[UC], int (&v)[UC][MAXDC]) {
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const int p = p0 + u * T;
            d[u] = 0;
#pragma unroll
            for (int j = 0; j < MAXDC; ++j) {
                const bool has = p < row[j + 1] - row[j];
                v[u][j] = has ? a.var[row[j] + p] : 0;
                d[u] += has;
            }
        }
    };
    // One step of a layer: UC checks of this thread, every load issued before the first use.
    // fast: every word the layer touches is in LDS (always so in the LDS form, and in the slab
    // form for the layers whose messages lie below lds_slots) -- the reads are then unconditional
    // ds_reads (an absent edge reads word 0) instead of one masked branch per word.
    auto step = [&](auto fast, const int32_t *row, int p0, const int (&d)[UC], const int (&v)[UC][MAXDC]) {
        constexpr bool FAST = decltype(fast)::value;
        float x[UC][MAXDC], xo[UC][MAXDC], r[UC][MAXDC];
#pragma unroll
        for (int u = 0; u < UC; ++u)
#pragma unroll
            for (int j = 0; j < MAXDC; ++j) {
                const bool has = j < d[u];
                if constexpr (FAST) {
                    const float pv = blk_l[v[u][j]], rv = blk_l[has ? n + row[j] + p0 + u * T : 0];
                    x[u][j] = has ? pv : __builtin_inff();
                    r[u][j] = has ? rv : 0.0f;
                } else {
                    x[u][j] = has ? LD(v[u][j]) : __builtin_inff();
                    r[u][j] = has ? LD(n + row[j] + p0 + u * T) : 0.0f;
                }
            }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (d[u] == 0) continue;  // no check at this position
#pragma unroll
            for (int j = 0; j < MAXDC; ++j) xo[u][j] = x[u][j] = x[u][j] - r[u][j];
            check_update<ALGO, MAXDC>(x[u], a.alpha, d[u]);
#pragma unroll
            for (int j = 0; j < MAXDC; ++j)
                if (j < d[u]) {
                    if constexpr (FAST) {
                        blk_l[n + row[j] + p0 + u * T] = x[u][j];
                        blk_l[v[u][j]] = xo[u][j] + x[u][j];
                    } else {
                        ST(n + row[j] + p0 + u * T, x[u][j]);
                        ST(v[u][j], xo[u][j] + x[u][j]);
                    }
                }
        }
    };
    // the first step of the next layer, loaded ahead of the barrier that ends this one (the index
    // reads wait for nothing the layer writes); at check degrees above 8 the registers go to the
    // check rule (the 16-wide slab form spilled and lost a quarter of its rate with it)
    constexpr bool PF = MAXDC <= 8;
    int dn[UC], vn[UC][MAXDC];

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        __syncthreads();  // previous codeword fully drained
        if (MC) {
            for (int i = tid; i <= iters; i += T) curve[i] = 0;
        }
        int err0 = 0;
        for (int v = tid; v < n; v += T) {
            const float l = MC ? chan_soft(a.ch, cw, v) : a.llr[(size_t)b * n + v];
            ST(v, to_msg<ALGO>(l));
            err0 += (l < 0.0f);
            if (!MC && iters == 0) {  // no iteration: the channel values themselves
                if (a.post) a.post[(size_t)b * n + v] = l;
                if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(l < 0.0f);
            }
        }
        for (int e = tid; e < E; e += T) ST(n + e, 0.0f);
        __syncthreads();
        count(0, err0);
        int it = 0;
        if constexpr (PF) load_vars(a.tab, tid, dn, vn);
        while (it < iters) {
            for (int l = 0; l < L; ++l) {
                const int32_t *row = a.tab + (size_t)l * kLayerTab;  // wave-uniform: scalar loads
                const int cnt = row[1] - row[0];                     // every check has a first edge
                auto steps = [&](auto fast) {
                    int p0 = tid;
                    if constexpr (PF) {  // the first step's indices are here already
                        step(fast, row, p0, dn, vn);
                        p0 += T * UC;
                    }
                    for (; p0 < cnt; p0 += T * UC) {
                        int d[UC], v[UC][MAXDC];
                        load_vars(row, p0, d, v);
                        step(fast, row, p0, d, v);
                    }
                };
                if constexpr (!GMEM) {
                    steps(bool_c<true>());
                } else {
                    if (n + row[MAXDC] <= S) steps(bool_c<true>());  // wave-uniform: the layer's last word
                    else steps(bool_c<false>());
                }
                // the next layer's first step (after the last layer: the next iteration's or codeword's)
                if constexpr (PF) load_vars(a.tab + (size_t)(l + 1 == L ? 0 : l + 1) * kLayerTab, tid, dn, vn);
                __syncthreads();  // the layer's posteriors, before the next layer gathers them
            }
            ++it;
            if (MC) {
                int errs = 0;
                for (int v = tid; v < n; v += T) errs += (LD(v) < 0.0f);
                count(it, errs);
            }
            if constexpr (ET) {
                // the syndrome of the decisions, on the layers' tables (nothing is written: no barrier between layers)
                int unsat = 0;
                for (int l = 0; l < L; ++l) {
                    const int32_t *row = a.tab + (size_t)l * kLayerTab;
                    const int cnt = row[1] - row[0];
                    for (int p = tid; p < cnt; p += T) {
                        int vv[MAXDC];
#pragma unroll
                        for (int j = 0; j < MAXDC; ++j) vv[j] = p < row[j + 1] - row[j] ? a.var[row[j] + p] : -1;
                        int par = 0;
                        if (!GMEM || n <= S) {  // every posterior in LDS: unconditional reads
#pragma unroll
                            for (int j = 0; j < MAXDC; ++j) par ^= (int)(vv[j] >= 0) & (int)(blk_l[max(vv[j], 0)] < 0.0f);
                        } else {
#pragma unroll
                            for (int j = 0; j < MAXDC; ++j)
                                if (vv[j] >= 0) par ^= (int)(LD(vv[j]) < 0.0f);
                        }
                        unsat |= par;
                    }
                }
                if (!__syncthreads_or(unsat)) break;
            } else if (MC) {
                __syncthreads();  // the count has read P: the next iteration's first layer may write it
            }
        }
        __syncthreads();
        if (!MC && iters > 0) {
            for (int v = tid; v < n; v += T) {
                const float s = LD(v);
                if (a.post) a.post[(size_t)b * n + v] = s * Domain<ALGO>::out;
                if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(s < 0.0f);
            }
        }
        if (MC) {
            int32_t *tr = a.trial + (size_t)b * (iters + 1);
            const int last = curve[it];
            for (int i = tid; i <= iters; i += T) tr[i] = i <= it ? curve[i] : last;
        }
        if ((MC || a.its) && tid == 0) a.its[b] = it;
    }
}

template <int MAXDC, int ALGO, bool ET, bool MC, bool GMEM>
hipError_t launch_layer_shape(const BpPlan &p, LayerArgs a, hipStream_t s) {
    constexpr int T = GMEM ? LDPC_GMEM_T : 256;
    if (p.threads != T) return hipErrorInvalidValue;
    auto k = bp_layer_kernel<T, MAXDC, ALGO, ET, MC, GMEM>;
    a.lds_slots = p.lds_slots;
    return launch_lds(k, dim3(p.grid), dim3(T), p.lds, s, a);
}

}  // namespace

hipError_t launch_layer(const BpPlan &p, LayerArgs a, int algo, bool et, bool mc, hipStream_t s) {
    return bp_modes(algo, et, mc, [&](auto A, auto Et, auto M) {
        constexpr int ALGO = decltype(A)::value;
        constexpr bool ET = decltype(Et)::value, MC = decltype(M)::value;
        switch (p.path) {
            case BpPath::Layer8: return launch_layer_shape<8, ALGO, ET, MC, false>(p, a, s);
            case BpPath::Layer16: return launch_layer_shape<16, ALGO, ET, MC, false>(p, a, s);
            case BpPath::Layer32: return launch_layer_shape<32, ALGO, ET, MC, false>(p, a, s);
            case BpPath::LayerG8: return launch_layer_shape<8, ALGO, ET, MC, true>(p, a, s);
            case BpPath::LayerG16: return launch_layer_shape<16, ALGO, ET, MC, true>(p, a, s);
            case BpPath::LayerG32: return launch_layer_shape<32, ALGO, ET, MC, true>(p, a, s);
            default: return hipErrorNotSupported;
        }
    });
}

}  // namespace ldpc
