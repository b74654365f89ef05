// ML ("optimal") erasure decoding.
//
// Reference behaviour restated here:
//   parallel_simulator.py:60-129   -> ml_kernel (ML erasure decoding, optimal_decode)
#include <algorithm>

#include "device_common.hpp"
#include "ldpc_internal.hpp"

namespace ldpc {
namespace {

// ===========================================================================
// 6. ML ("optimal") erasure decoding -- optimal_decode, parallel_simulator.py:60-129
//    (system set-up of ml_decoder.c:7-36, GF(2) row_reduce of the galois package)
// ===========================================================================
//
// One workgroup per word.  Thread t holds ROW POSITION t of the augmented system
// [A | target] in registers as W 64-bit words (A = H restricted to the erased
// columns that are still unknown, target = parity of the known 1-bits of each
// active check), so elimination needs no LDS for the matrix: per column j one
// ballot + LDS atomicMin finds the pivot row (first position >= j with bit j set,
// galois' choice); each wave's first candidate row is staged in LDS before the
// barrier, so one barrier per column suffices; rows p and q swap through LDS, and
// every other row holding bit j XORs the pivot in (Gauss-Jordan, above and below).
// Because the reference looks for the FIRST column whose diagonal entry of the
// reduced matrix is not 1, elimination stops at the first column without a pivot
// (all earlier columns are pivots, so that column IS the first diagonal miss):
// that unknown is given up, every check holding it is dropped, and the system is
// rebuilt from the graph and reduced again -- the reference's loop (:93-108).
// When every remaining column has a pivot the solution is read off the augmented
// bit of rows 0..ncols-1 (:110-121).  Words with no erasure or more erasures than
// checks are returned unchanged (:66-70).  m <= 1000 (the 1000-unknown cap of
// :96 can then never bind); n <= 32767.
//
// Per-word LDS (dynamic): cand[2][T/64][W], swp[2][W] (u64); best[3], wsum[16] (int);
// code[n] (int16: column of an active unknown, -1/-2 known 0/1, -3 given up);
// state[n] (u8: 0/1 known, 2 unknown, 3 given up, 4/5 solved 0/1);
// rowchk[m], colvar[m] (int16); achk[m] (u8).

// Register-array helpers with static indices only (a data-dependent index would
// push R[] to scratch): set bit k by masks, and drop the front word (the
// elimination window: columns left of the current 64-column block are never read
// again, and every row's bit j sits in word 0).
template <int W>
__device__ __forceinline__ void ml_set_bit(uint64_t (&R)[W], int k) {
    const int kw = k >> 6;
    const uint64_t b = 1ull << (k & 63);
#pragma unroll
    for (int w = 0; w < W; ++w) R[w] |= (0ull - (uint64_t)(kw == w)) & b;
}

template <int W>
__device__ __forceinline__ void ml_shift(uint64_t (&R)[W]) {
#pragma unroll
    for (int w = 0; w + 1 < W; ++w) R[w] = R[w + 1];
    R[W - 1] = 0;
}

// cptr == nullptr: regular lists, check c owns slots [c*dc, c*dc+dc) of
// cvar + b*cvar_stride (ensemble mode: word b decodes on its own graph b).
template <int W>
__global__ __launch_bounds__(1024) void ml_kernel(const int32_t *__restrict__ cptr, const int32_t *__restrict__ cvar,
                                                  int64_t cvar_stride, int dc, int n, int m,
                                                  const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                  int32_t *__restrict__ unsolved) {
    extern __shared__ __align__(16) unsigned char ml_lds[];
    const int NW = blockDim.x >> 6;
    uint64_t *cand = reinterpret_cast<uint64_t *>(ml_lds);  // [2][NW][W] each wave's first candidate row
    uint64_t *swp = cand + 2 * NW * W;                       // [2][W] row at the pivot position
    int *best = reinterpret_cast<int *>(swp + 2 * W);        // [3]
    int *wsum = best + 3;                                    // [16]
    int16_t *code = reinterpret_cast<int16_t *>(wsum + 16); // [n]
    int16_t *rowchk = code + n;                             // [m]
    int16_t *colvar = rowchk + m;                           // [m]
    uint8_t *state = reinterpret_cast<uint8_t *>(colvar + m);  // [n]
    uint8_t *achk = state + n;                              // [m]

    const int tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const uint8_t *w_in = in + b * n;
    uint8_t *w_out = out + b * n;
    const int32_t *gv = cvar + (int64_t)b * cvar_stride;

    int ne_local = 0;
    for (int v = tid; v < n; v += T) {
        const uint8_t x = w_in[v];
        state[v] = x == 2 ? 2 : (x ? 1 : 0);
        ne_local += (x == 2);
    }
    for (int c = tid; c < m; c += T) achk[c] = 1;
    if (tid < 3) best[tid] = INT_MAX;
    int ne = 0;
    (void)block_excl_scan(ne_local, wsum, ne);  // (its barriers also publish state / achk / best)
    if (ne == 0 || ne > m) {
        for (int v = tid; v < n; v += T) w_out[v] = w_in[v];
        if (tid == 0) unsolved[b] = ne;
        return;
    }
    const int vper = (n + T - 1) / T, cper = (m + T - 1) / T;
    int marks = 0;
    for (;;) {
        // --- columns: the active unknowns in position order
        const int v0 = min(n, tid * vper), v1 = min(n, v0 + vper);
        int cnt = 0;
        for (int v = v0; v < v1; ++v) cnt += (state[v] == 2);
        int ncols = 0;
        int col = block_excl_scan(cnt, wsum, ncols);
        for (int v = v0; v < v1; ++v) {
            const int st = state[v];
            if (st == 2) {
                colvar[col] = (int16_t)v;
                code[v] = (int16_t)col++;
            } else {
                code[v] = (int16_t)(st == 3 ? -3 : -1 - st);
            }
        }
        // --- rows: the active checks in index order
        const int c0 = min(m, tid * cper), c1 = min(m, c0 + cper);
        cnt = 0;
        for (int c = c0; c < c1; ++c) cnt += achk[c];
        int nrows = 0;
        int pos = block_excl_scan(cnt, wsum, nrows);  // barrier: code[] / colvar[] complete
        for (int c = c0; c < c1; ++c)
            if (achk[c]) rowchk[pos++] = (int16_t)c;
        __syncthreads();
        // --- build row `tid` of [A | target]
        uint64_t R[W];
#pragma unroll
        for (int w = 0; w < W; ++w) R[w] = 0;
        int s_lo = 0, s_hi = 0;
        if (tid < nrows) {
            const int c = rowchk[tid];
            s_lo = cptr ? cptr[c] : c * dc;
            s_hi = cptr ? cptr[c + 1] : s_lo + dc;
            int tgt = 0;
            for (int s = s_lo; s < s_hi; ++s) {
                const int v = gv[s];
                const int k = code[v];
                if (k >= 0) {
                    ml_set_bit<W>(R, k);  // H is a 0/1 matrix: set, not toggle
                } else if (k == -2) {
                    bool dup = false;     // a variable listed twice in a check counts once
                    for (int s2 = s_lo; s2 < s; ++s2) dup |= (gv[s2] == v);
                    tgt ^= dup ? 0 : 1;
                }
            }
            if (tgt) ml_set_bit<W>(R, ncols);
        }
        // --- Gauss-Jordan in galois' pivot order until the first column without a pivot.
        // Window: R[0] holds columns [64*shift, 64*shift+64) of the row.  One barrier
        // per column: every wave's first candidate row is published before the barrier
        // (with the row at the pivot position, for the swap), so the winner's row is
        // already in LDS once the pivot position is known.  cand/swp are double-
        // buffered by column parity, best[] triple-buffered (the atomicMin of column
        // j+1 may run before a slow thread reads best[] of column j).
        int free_col = -1, shift = 0, b3 = 0, j = 0;
        // One 64-column block at a time with the L = live words of the window only
        // (words past the augmented column are zero in every row), so the column
        // step is branch-free and its cost shrinks as the elimination advances.
        auto block = [&](auto live_tag) {
            constexpr int L = decltype(live_tag)::value;
            const int jend = min(ncols, 64 * (shift + 1));
            for (; j < jend; ++j) {
                const int buf = j & 1;
                const bool bit = (R[0] >> (j & 63)) & 1ull;
                const uint64_t bal = __ballot(bit && tid >= j && tid < nrows);
                if (bal && lane == (int)__ffsll((long long)bal) - 1) {
                    uint64_t *cw = cand + (buf * NW + wave) * W;
#pragma unroll
                    for (int w = 0; w < L; ++w) cw[w] = R[w];
                    atomicMin(&best[b3], tid);
                }
                if (tid == j) {
#pragma unroll
                    for (int w = 0; w < L; ++w) swp[buf * W + w] = R[w];
                }
                __syncthreads();
                const int q = best[b3];
                const int b_old = b3 == 0 ? 2 : b3 - 1;  // buffer of column j-1 == column j+2
                if (tid == 0) best[b_old] = INT_MAX;
                b3 = b3 == 2 ? 0 : b3 + 1;
                if (q == INT_MAX) {
                    free_col = j;
                    return;
                }
                const uint64_t *pb = cand + (buf * NW + (q >> 6)) * W;
                const bool take = (tid == j) && (q != j);               // row j becomes the pivot row
                const uint64_t msk = (bit && tid != q) ? ~0ull : 0ull;  // rows holding bit j XOR it in
#pragma unroll
                for (int w = 0; w < L; ++w) {
                    const uint64_t pw = pb[w];
                    R[w] = take ? pw : (R[w] ^ (pw & msk));
                }
                if (tid == q && q != j) {  // the old row j moves to position q
#pragma unroll
                    for (int w = 0; w < L; ++w) R[w] = swp[buf * W + w];
                }
            }
            if (j < ncols) {  // next block: drop the front word
#pragma unroll
                for (int w = 0; w + 1 < L; ++w) R[w] = R[w + 1];
                R[L - 1] = 0;
                ++shift;
            }
        };
        while (j < ncols && free_col < 0) {
            switch (min(W, (ncols >> 6) - shift + 1)) {  // live words: columns [64*shift, ncols]
#define LDPC_ML_LIVE(LL) \
    case LL:             \
        if constexpr (LL <= W) block(std::integral_constant<int, LL>{}); \
        break;
                LDPC_ML_LIVE(1) LDPC_ML_LIVE(2) LDPC_ML_LIVE(3) LDPC_ML_LIVE(4)
                LDPC_ML_LIVE(5) LDPC_ML_LIVE(6) LDPC_ML_LIVE(7) LDPC_ML_LIVE(8)
                LDPC_ML_LIVE(9) LDPC_ML_LIVE(10) LDPC_ML_LIVE(11) LDPC_ML_LIVE(12)
                LDPC_ML_LIVE(13) LDPC_ML_LIVE(14) LDPC_ML_LIVE(15) LDPC_ML_LIVE(16)
#undef LDPC_ML_LIVE
                default: block(std::integral_constant<int, W>{});
            }
        }
        if (free_col < 0) {
            // full column rank: unknown j = augmented bit (column ncols) of row j
            while (shift < (ncols >> 6)) {
                ml_shift<W>(R);
                ++shift;
            }
            if (tid < ncols) {
                const int v = colvar[tid];
                state[v] = (uint8_t)(4 + ((R[0] >> (ncols & 63)) & 1ull));
            }
            __syncthreads();
            break;
        }
        // --- give the unknown up: drop it and every check that holds it
        const int vf = colvar[free_col];
        if (tid < nrows) {
            bool has = false;
            for (int s = s_lo; s < s_hi; ++s) has |= (gv[s] == vf);
            if (has) achk[rowchk[tid]] = 0;
        }
        if (tid == 0) state[vf] = 3;
        ++marks;
        __syncthreads();
    }
    for (int v = tid; v < n; v += T) {
        const int st = state[v];
        w_out[v] = st == 3 ? 2 : (st >= 4 ? (uint8_t)(st - 4) : w_in[v]);
    }
    if (tid == 0) unsolved[b] = marks;
}

size_t ml_lds_bytes(int n, int m, int W, int T) {
    return (size_t)8 * (2 * (T / 64) + 2) * W + 4 * 19 + (size_t)2 * n + (size_t)4 * m + (size_t)n + (size_t)m + 16;
}

int ml_words(int m) {
    const int need = (m + 1 + 63) / 64;
    for (int w : {1, 2, 4, 8, 16})
        if (w >= need) return w;
    return 0;
}

}  // namespace

hipError_t launch_ml_decode(const int32_t *cptr, const int32_t *cvar, int64_t cvar_stride, int dc, int n, int m,
                            const uint8_t *d_in, int B, uint8_t *d_out, int32_t *d_unsolved, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    const int W = ml_words(m);
    const int T = std::min(1024, std::max(64, (m + 63) / 64 * 64));
    const size_t lds = ml_lds_bytes(n, m, W, T);
#define LDPC_ML_CASE(WW)                                                                                        \
    case WW:                                                                                                    \
        return launch_lds(ml_kernel<WW>, dim3(B), dim3(T), lds, stream, cptr, cvar, cvar_stride, dc, n, m, d_in, \
                          d_out, d_unsolved);
    switch (W) {
        LDPC_ML_CASE(1)
        LDPC_ML_CASE(2)
        LDPC_ML_CASE(4)
        LDPC_ML_CASE(8)
        LDPC_ML_CASE(16)
        default: return hipErrorInvalidValue;
    }
#undef LDPC_ML_CASE
}

}  // namespace ldpc
