// bp_qc_q_kernel: the fixed-point layered min-sum of bp_layer_q.hip on a quasi-cyclic code, where
// H is an mb x nb array of Z x Z circulant permutations or zero blocks, and its launch ladder.
// Semantics: include/ldpc_mi355x.h, ldpc_bp_layered_q_decode_batch_dev -- every value an integer,
// so the kernel is bit-exact with that text, and with bp_layer_q_kernel on the same graph.
//
// Block, record format, quantiser, check step, early stop, Monte-Carlo curve and outputs are
// bp_layer_q_kernel's (bp_layer_q.hpp):
//   curve | posteriors P int8[n] (padded to 4 bytes) | one record per check, the record of check c at c
// What differs: a block row is a layer (its Z checks share no variable), and check r Z + i holds
// variable c Z + (i + s_rc) mod Z for every non-zero cell of block row r in ascending block-column
// order (the expansion convention of the header, ldpc_graph_create_qc).  So thread i takes checks
// i, i + T, ... < Z of the row and forms its variables in registers from the row's degree and
// (column base, shift) pairs -- wave-uniform loads from the row table (kQcRow) -- with no index
// table read, and lanes i, i + 1, ... of a wave read neighbouring bytes of P.  The row's degree is
// the same for every lane.  One workgroup barrier ends a block row.
#include "bp_layer_q.hpp"

namespace ldpc {
namespace {

// Cw: nothing, or one CwArgs behind the plain arguments -- the codeword mode (only with MC), as in
// bp_layer_q.hip: cw_stage, cw_count and the bit plane after the records (bp_layer_q.hpp).
template <int T, int MAXDC, bool ET, bool MC, typename... Cw>
__global__ __launch_bounds__(T) void bp_qc_q_kernel(QcQArgs qa, Cw... cwa) {
    constexpr bool CW = sizeof...(Cw) > 0;
    static_assert(MC || !CW, "the codeword mode is a Monte-Carlo mode");
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int RW = MAXDC <= 16 ? 1 : 2;  // words of a record
    const LayerQArgs &a = qa.q;
    const int tid = threadIdx.x;
    const int n = a.n, m = a.m, iters = a.max_iters, mb = a.L, Z = qa.Z;
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
    const LayerQStep<MAXDC> step{P, rec, Q, Pmax, norm8, offset};
    // Variables of check p < Z of a block row (an entry past the row's degree: base 0, shift 0,
    // so variable p, which is not used)
    auto row_vars = [&](const int32_t *row, int p, int (&v)[MAXDC]) {
#pragma unroll
        for (int j = 0; j < MAXDC; ++j) {
            const int t = p + row[2 + 2 * j];
            v[j] = row[1 + 2 * j] + t - (t >= Z ? Z : 0);
        }
    };
    // negative bytes of P word w (the padding bytes stay 0)
    auto neg_bytes = [&](int w) { return __builtin_popcount(Pw[w] & 0x80808080u); };

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
        while (it < iters) {
            for (int r = 0; r < mb; ++r) {
                const int32_t *row = qa.row + (size_t)r * kQcRow;  // wave-uniform: scalar loads
                const int d = row[0], cb = r * Z;
                for (int p = tid; p < Z; p += T) {
                    int v[MAXDC];
                    row_vars(row, p, v);
                    step(cb + p, d, v);
                }
                __syncthreads();  // the block row's posteriors, before the next one gathers them
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
                // the syndrome of the decisions, on the same indices (nothing is written: no barrier between rows)
                int unsat = 0;
                for (int r = 0; r < mb; ++r) {
                    const int32_t *row = qa.row + (size_t)r * kQcRow;
                    const int d = row[0];
                    for (int p = tid; p < Z; p += T) {
                        int v[MAXDC];
                        row_vars(row, p, v);
                        int par = 0;
#pragma unroll
                        for (int j = 0; j < MAXDC; ++j) par ^= (int)(j < d) & (int)(P[v[j]] < 0);
                        unsat |= par;
                    }
                }
                if (!__syncthreads_or(unsat)) break;
            } else if (MC) {
                __syncthreads();  // the count has read P: the next iteration's first row may write it
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

template <int T, int MAXDC>
hipError_t launch_qc_q_shape(const BpPlan &p, const QcQArgs &a, bool et, bool mc, const CwArgs *cw, hipStream_t s) {
    if (p.threads != T) return hipErrorInvalidValue;
    if (cw) {  // the codeword mode: Monte-Carlo only
        if (!mc) return hipErrorInvalidValue;
        auto go = [&](auto k) { return launch_lds(k, dim3(p.grid), dim3(T), p.lds, s, a, *cw); };
        return et ? go(bp_qc_q_kernel<T, MAXDC, true, true, CwArgs>) : go(bp_qc_q_kernel<T, MAXDC, false, true, CwArgs>);
    }
    auto go = [&](auto k) { return launch_lds(k, dim3(p.grid), dim3(T), p.lds, s, a); };
    if (et) return mc ? go(bp_qc_q_kernel<T, MAXDC, true, true>) : go(bp_qc_q_kernel<T, MAXDC, true, false>);
    return mc ? go(bp_qc_q_kernel<T, MAXDC, false, true>) : go(bp_qc_q_kernel<T, MAXDC, false, false>);
}

}  // namespace

hipError_t launch_qc_q(const BpPlan &p, const QcQArgs &a, bool et, bool mc, const CwArgs *cw, hipStream_t s) {
    switch (p.path) {
#define LDPC_ROW(T, D) \
    case BpPath::QcQ##T##x##D: return launch_qc_q_shape<T, D>(p, a, et, mc, cw, s);
        LDPC_QC_Q_SHAPES(LDPC_ROW)
#undef LDPC_ROW
        default: return hipErrorNotSupported;
    }
}

}  // namespace ldpc
