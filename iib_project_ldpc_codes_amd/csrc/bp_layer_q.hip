// bp_layer_q_kernel: fixed-point layered min-sum with compressed check records, on any graph with
// a layer schedule whose block fits LDS (bp_layer_q_plan), and its launch ladder.  Semantics:
// include/ldpc_mi355x.h, ldpc_bp_layered_q_decode_batch_dev -- every value an integer, so the
// kernel is bit-exact with that text.
//
// One workgroup decodes one codeword at a time on a block
//   posteriors P int8[n] (padded to 4 bytes) | one record per check, in layer order
// in LDS (the record's format, the quantiser and the step of one check: bp_layer_q.hpp, shared with
// bp_qc_q.hip).  Record lay_cbase[l] + p belongs to the check at position p of layer l,
// so the threads of a wave read neighbouring records.  As in bp_layer.hip thread i takes positions
// i, i + T, ... of a layer and one workgroup barrier ends the layer; the checks of a layer share no
// variable, so the byte stores to P of different threads never touch the same byte.
#include "bp_layer_q.hpp"

namespace ldpc {
namespace {

// Cw: nothing, or one CwArgs behind the plain arguments -- the codeword mode (only with MC):
// cw_stage in place of the fused channel, cw_count in place of the count of negative bytes, the bit
// plane after the records (bp_layer_q.hpp); the loop is the same.
template <int T, int MAXDC, bool ET, bool MC, typename... Cw>
__global__ __launch_bounds__(T) void bp_layer_q_kernel(LayerQArgs a, Cw... cwa) {
    constexpr bool CW = sizeof...(Cw) > 0;
    static_assert(MC || !CW, "the codeword mode is a Monte-Carlo mode");
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int RW = MAXDC <= 16 ? 1 : 2;  // words of a record
    const int tid = threadIdx.x;
    const int n = a.n, m = a.m, iters = a.max_iters, L = a.L;
    const int Q = a.Q, Pmax = a.Pmax, norm8 = a.norm8, offset = a.offset;
    const int n4 = (n + 3) >> 2;  // words of P
    // LDS: curve (16-byte padded, Monte-Carlo only) | P | records
    const size_t curve_pad = MC ? curve_bytes(iters) : 0;
    int *curve = reinterpret_cast<int *>(smem);
    lds_i8 *P = (lds_i8 *)((lds_u8 *)smem + curve_pad);
    lds_u32 *Pw = (lds_u32 *)P;
    lds_u32 *rec = Pw + n4;
    // Monte-Carlo: bit errors of the workgroup's decisions into curve[i]
    auto count = [&](int i, int errs) {
        if (MC) {
            const int w = wave_sum(errs);
            if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[i], w);
        }
    };

    // Variables and degree of the check at position p of a layer (bp_layer.hip's load_vars)
    auto load_vars = [&](const int32_t *row, int p, int &d, int (&v)[MAXDC]) {
        d = 0;
#pragma unroll
        for (int j = 0; j < MAXDC; ++j) {
            const bool has = p < row[j + 1] - row[j];
            v[j] = has ? a.var[row[j] + p] : 0;
            d += has;
        }
    };
    // The check with record c, degree d > 0 and variables v (layer_q_step, bp_layer_q.hpp)
    const LayerQStep<MAXDC> step{P, rec, Q, Pmax, norm8, offset};
    // negative bytes of P word w (the padding bytes stay 0)
    auto neg_bytes = [&](int w) { return __builtin_popcount(Pw[w] & 0x80808080u); };
    // the first step of the next layer, loaded ahead of the barrier that ends this one (the index
    // reads wait for nothing the layer writes); above degree 8 the registers go to the check rule
    constexpr bool PF = MAXDC <= 8;
    int dn = 0, vn[MAXDC];

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        __syncthreads();  // previous codeword fully drained
        if (MC) {
            for (int i = tid; i <= iters; i += T) curve[i] = 0;
        }
        int err0 = 0;
        if constexpr (CW) {
            err0 = cw_stage<T>(a, cw_args(cwa...), b, cw, Pw, rec + m * RW);
        } else {
            for (int v = n + tid; v < 4 * n4; v += T) P[v] = 0;  // the padding bytes
            for (int v = tid; v < n; v += T) {
                const float l = MC ? chan_soft(a.ch, cw, v) : a.llr[(size_t)b * n + v];
                const int c = quantise(l, a.scale, Q);
                P[v] = (signed char)c;
                err0 += (c < 0);
                if (!MC && iters == 0) {  // no iteration: the quantised channel values themselves
                    if (a.post) a.post[(size_t)b * n + v] = (int8_t)c;
                    if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(c < 0);
                }
            }
        }
        for (int i = tid; i < m * RW; i += T) rec[i] = 0;  // R = 0
        __syncthreads();
        count(0, err0);
        int it = 0;
        if constexpr (PF) load_vars(a.tab, tid, dn, vn);
        while (it < iters) {
            for (int l = 0; l < L; ++l) {
                const int32_t *row = a.tab + (size_t)l * kLayerTab;  // wave-uniform: scalar loads
                const int cnt = row[1] - row[0];                     // every check has a first edge
                const int cb = a.cbase[l];
                int p = tid;
                if constexpr (PF) {  // the first step's indices are here already
                    if (dn > 0) step(cb + p, dn, vn);
                    p += T;
                }
                for (; p < cnt; p += T) {
                    int d, v[MAXDC];
                    load_vars(row, p, d, v);
                    step(cb + p, d, v);
                }
                // the next layer's first step (after the last layer: the next iteration's or codeword's)
                if constexpr (PF) load_vars(a.tab + (size_t)(l + 1 == L ? 0 : l + 1) * kLayerTab, tid, dn, vn);
                __syncthreads();  // the layer's posteriors, before the next layer gathers them
            }
            ++it;
            if (MC) {
                int errs = 0;
                if constexpr (CW) {  // against the codeword's plane, under the description's count mask
                    errs = cw_count<T>(Pw, rec + m * RW, cw_args(cwa...).desc, n4);
                } else {
                    for (int w = tid; w < n4; w += T) errs += neg_bytes(w);
                }
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
#pragma unroll
                        for (int j = 0; j < MAXDC; ++j) par ^= (int)(vv[j] >= 0) & (int)(P[max(vv[j], 0)] < 0);
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
                const int s = P[v];
                if (a.post) a.post[(size_t)b * n + v] = (int8_t)s;
                if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(s < 0);
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

template <int MAXDC>
hipError_t launch_layer_q_shape(const BpPlan &p, const LayerQArgs &a, bool et, bool mc, const CwArgs *cw,
                                hipStream_t s) {
    constexpr int T = 256;
    if (p.threads != T) return hipErrorInvalidValue;
    if (cw) {  // the codeword mode: Monte-Carlo only
        if (!mc) return hipErrorInvalidValue;
        auto go = [&](auto k) { return launch_lds(k, dim3(p.grid), dim3(T), p.lds, s, a, *cw); };
        return et ? go(bp_layer_q_kernel<T, MAXDC, true, true, CwArgs>)
                  : go(bp_layer_q_kernel<T, MAXDC, false, true, CwArgs>);
    }
    auto go = [&](auto k) { return launch_lds(k, dim3(p.grid), dim3(T), p.lds, s, a); };
    if (et) return mc ? go(bp_layer_q_kernel<T, MAXDC, true, true>) : go(bp_layer_q_kernel<T, MAXDC, true, false>);
    return mc ? go(bp_layer_q_kernel<T, MAXDC, false, true>) : go(bp_layer_q_kernel<T, MAXDC, false, false>);
}

}  // namespace

hipError_t launch_layer_q(const BpPlan &p, const LayerQArgs &a, bool et, bool mc, const CwArgs *cw, hipStream_t s) {
    switch (p.path) {
        case BpPath::LayerQ8: return launch_layer_q_shape<8>(p, a, et, mc, cw, s);
        case BpPath::LayerQ16: return launch_layer_q_shape<16>(p, a, et, mc, cw, s);
        case BpPath::LayerQ32: return launch_layer_q_shape<32>(p, a, et, mc, cw, s);
        default: return hipErrorNotSupported;
    }
}

}  // namespace ldpc
