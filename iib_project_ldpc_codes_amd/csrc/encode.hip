// The codeword family: systematic encoding, the information-bit stream, the channel of a
// transmitted codeword and the error counts against it.  The C ABI's ldpc_encode_batch_dev,
// ldpc_info_bits_dev, ldpc_channel_cw_dev and ldpc_mc_cw_count_dev (include/ldpc_mi355x.h) launch
// these; none of the fused all-zero kernels is involved.
//
// Encoding is P = A U over GF(2), bit-sliced: a plane word holds one bit position of 32 codewords
// (bit i = codeword i of the word), as in gb.hip and bec.hip.
//
// encode_parity_kernel<W>: one workgroup takes a tile of 32 W codewords (encode_plan.cpp picks W).
//   LDS  U[K][W]: the tile's information planes, packed from the info bytes (bit 0 read).
//   One thread works on one row of A, in row blocks of the workgroup size, and loops j over K: the
//   A word comes from the transposed copy At[j >> 5][row] (a wave's loads coalesce), U[j] is one LDS
//   address for the whole wave (a broadcast read), acc[w] ^= -bit & U[j][w] (one v_bitop3_b32).
//   The W parity words of the row go to planes[tile W + w][row]: coalesced over the rows of a wave.
// encode_write_kernel: a thread owns four consecutive variables of one codeword, takes each from the
//   info bytes or from its parity plane word (src[v]) and stores them as one dword (bytes when n is
//   no multiple of 4 or the output is not 4-byte aligned).
#include "channel_cw.hpp"
#include "device_common.hpp"
#include "ldpc_internal.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {
namespace {

// a ^ (b & c) in one v_bitop3_b32: truth table 0xF0 ^ (0xCC & 0xAA)
__device__ __forceinline__ uint32_t xor_and(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x78);
}

template <int W>
__global__ __launch_bounds__(1024) void encode_parity_kernel(const uint32_t *__restrict__ At,
                                                             const uint8_t *__restrict__ info, int K, int KW, int rank,
                                                             int B, uint32_t *__restrict__ planes) {
    extern __shared__ __align__(16) uint32_t U[];  // [K][W]
    const int tid = threadIdx.x, T = blockDim.x;
    const int64_t cw0 = (int64_t)blockIdx.x * (32 * W);
    for (int j = tid; j < K; j += T) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            uint32_t word = 0u;
            const int64_t c0 = cw0 + 32 * w;
            const int nb = (int)min((int64_t)32, (int64_t)B - c0);  // <= 0: a plane word past the batch
            for (int i = 0; i < nb; ++i) word |= (uint32_t)(info[(size_t)(c0 + i) * K + j] & 1u) << i;
            U[j * W + w] = word;
        }
    }
    __syncthreads();
    for (int row = tid; row < rank; row += T) {
        uint32_t acc[W];
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = 0u;
        for (int jw = 0; jw < KW; ++jw) {
            const uint32_t a = At[(size_t)jw * rank + row];
            const uint32_t *u = U + (size_t)(32 * jw) * W;
            if (32 * jw + 32 <= K) {
#pragma unroll
                for (int b = 0; b < 32; ++b) {
                    const uint32_t mk = (uint32_t)((int32_t)(a << (31 - b)) >> 31);
#pragma unroll
                    for (int w = 0; w < W; ++w) acc[w] = xor_and(acc[w], mk, u[b * W + w]);
                }
            } else {
                for (int b = 0; b < K - 32 * jw; ++b) {
                    const uint32_t mk = (uint32_t)((int32_t)(a << (31 - b)) >> 31);
#pragma unroll
                    for (int w = 0; w < W; ++w) acc[w] = xor_and(acc[w], mk, u[b * W + w]);
                }
            }
        }
#pragma unroll
        for (int w = 0; w < W; ++w) planes[((size_t)blockIdx.x * W + w) * rank + row] = acc[w];
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void encode_write_kernel(const int32_t *__restrict__ src,
                                                           const uint8_t *__restrict__ info,
                                                           const uint32_t *__restrict__ planes, int n, int K, int rank,
                                                           int B, uint8_t *__restrict__ cw) {
    const int groups = (n + 3) >> 2;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)groups * B) return;
    const size_t b = idx / groups;
    const int g = (int)(idx % groups);
    const uint32_t *word = planes + (b >> 5) * (size_t)rank;
    const int sh = (int)(b & 31);
    uint32_t out = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = 4 * g + i;
        if (v >= n) break;
        const int s = src[v];
        const uint32_t bit = s >= 0 ? info[b * K + s] & 1u : word[~s] >> sh & 1u;
        if (VEC) out |= bit << (8 * i);
        else cw[b * n + v] = (uint8_t)bit;
    }
    if (VEC) reinterpret_cast<uint32_t *>(cw)[(b * n >> 2) + g] = out;  // n % 4 == 0, cw 4-byte aligned
}

// Bit j of trial t: bit j & 31 of word (j >> 5) & 3 of Philox {j >> 7, 1, t_lo, t_hi} under the
// channels' key (make_chan).  A thread draws the four bits 4g .. 4g + 3: they share a word.
template <bool VEC>
__global__ __launch_bounds__(256) void info_bits_kernel(uint32_t k0, uint32_t k1, uint64_t first_cw, int K, int B,
                                                        uint8_t *__restrict__ info) {
    const int groups = (K + 3) >> 2;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)groups * B) return;
    const size_t b = idx / groups;
    const int j0 = 4 * (int)(idx % groups);
    const uint64_t t = first_cw + (uint64_t)b;
    const uint4 r = philox_block((uint32_t)(j0 >> 7), 1u, (uint32_t)t, (uint32_t)(t >> 32), k0, k1);
    const uint32_t x = pick4(r, (j0 >> 5) & 3) >> (j0 & 31);
    if (VEC) {  // K % 4 == 0, info 4-byte aligned
        reinterpret_cast<uint32_t *>(info)[(b * K + j0) >> 2] =
            (x & 1u) | (x >> 1 & 1u) << 8 | (x >> 2 & 1u) << 16 | (x >> 3 & 1u) << 24;
    } else {
        for (int i = 0; i < 4 && j0 + i < K; ++i) info[b * K + j0 + i] = (uint8_t)(x >> i & 1u);
    }
}

// channel_kernel (mc_kernels.hip) word for word, then the reflection where the codeword bit is 1:
// the BEC keeps its erased positions and shows x elsewhere, the BSC and AWGN LLRs change sign.
// The arithmetic is channel_cw.hpp's, shared with channel_rm_kernel (rate_match.hip).
__global__ __launch_bounds__(256) void channel_cw_kernel(int kind, float p, float p2, uint64_t seed, uint64_t first_cw,
                                                         int n, int B, const uint8_t *__restrict__ cw, void *out) {
    const int groups = (n + 3) >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)groups * B) return;
    channel_cw_group(
        kind, p, p2, seed, first_cw, n, groups, idx, cw, [&](int, size_t o, uint8_t word) { static_cast<uint8_t *>(out)[o] = word; },
        [&](int, size_t o, float llr) { static_cast<float *>(out)[o] = llr; });
}

// One workgroup per trial: channel errors [llr < 0] != x (bits: bit 0 != x) and final errors hard != x
template <bool LLR>
__global__ __launch_bounds__(256) void cw_count_kernel(const uint8_t *__restrict__ cw, const void *__restrict__ chan,
                                                       const uint8_t *__restrict__ hard, int n, int iters,
                                                       int32_t *__restrict__ trial) {
    __shared__ int red[256 / kWave];
    const size_t base = (size_t)blockIdx.x * n;
    int ce = 0, fe = 0;
    for (int v = threadIdx.x; v < n; v += 256) {
        const uint32_t x = cw[base + v] & 1u;
        const uint32_t y = LLR ? (static_cast<const float *>(chan)[base + v] < 0.0f ? 1u : 0u)
                               : static_cast<const uint8_t *>(chan)[base + v] & 1u;
        ce += y != x;
        fe += (hard[base + v] & 1u) != x;
    }
    ce = block_sum<256>(ce, red);
    fe = block_sum<256>(fe, red);
    int32_t *row = trial + (size_t)blockIdx.x * (iters + 1);
    for (int t = 1 + threadIdx.x; t < iters; t += 256) row[t] = 0;
    if (threadIdx.x == 0) {
        row[0] = ce;
        row[iters] = fe;  // iters == 0: the one entry is the final count
    }
}

// The tiles: the rows of the shape table (kernel_shapes.hpp), from which encode_plan takes the W it names
hipError_t launch_parity(const EncodePlan &p, const ldpc_encoder &e, const uint8_t *d_info, int B, uint32_t *planes,
                         hipStream_t s) {
#define LDPC_ROW(WW)                                                                                                  \
    if (p.W == WW)                                                                                                    \
        return launch_lds(encode_parity_kernel<WW>, dim3((unsigned)p.grid), dim3(p.threads), p.lds, s, e.At, d_info, \
                          e.K, e.KW, e.rank, B, planes);
    LDPC_ENC_TILES(LDPC_ROW)
#undef LDPC_ROW
    return hipErrorInvalidValue;  // a tile without a row: the plan gives none
}

}  // namespace

hipError_t launch_encode(const EncodePlan &p, const ldpc_encoder &e, const uint8_t *d_info, int B, uint32_t *planes,
                         uint8_t *d_cw, hipStream_t stream) {
    if (B <= 0 || e.n <= 0) return hipSuccess;
    if (e.rank > 0) {
        const hipError_t err = launch_parity(p, e, d_info, B, planes, stream);
        if (err != hipSuccess) return err;
    }
    const bool vec = e.n % 4 == 0 && (reinterpret_cast<uintptr_t>(d_cw) & 3) == 0;
    auto kernel = vec ? encode_write_kernel<true> : encode_write_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.write_grid), dim3(256), 0, stream, e.src, d_info, planes, e.n, e.K,
                       e.rank, B, d_cw);
    return hipGetLastError();
}

hipError_t launch_info_bits(uint64_t seed, uint64_t first_cw, int K, int B, uint8_t *d_info, hipStream_t stream) {
    if (B <= 0 || K <= 0) return hipSuccess;
    const size_t total = (size_t)((K + 3) / 4) * (size_t)B;
    const bool vec = K % 4 == 0 && (reinterpret_cast<uintptr_t>(d_info) & 3) == 0;
    auto kernel = vec ? info_bits_kernel<true> : info_bits_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32), first_cw, K, B, d_info);
    return hipGetLastError();
}

hipError_t launch_channel_cw(int channel, float p, float p2, uint64_t seed, uint64_t first_cw, int n, int B,
                             const uint8_t *d_cw, void *d_out, hipStream_t stream) {
    if (B <= 0 || n <= 0) return hipSuccess;
    const size_t total = (size_t)((n + 3) / 4) * (size_t)B;
    hipLaunchKernelGGL(channel_cw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, channel, p, p2,
                       seed, first_cw, n, B, d_cw, d_out);
    return hipGetLastError();
}

hipError_t launch_cw_count(const uint8_t *d_cw, const void *d_chan, bool chan_is_llr, const uint8_t *d_hard, int n,
                           int B, int max_iters, int32_t *trial, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    auto kernel = chan_is_llr ? cw_count_kernel<true> : cw_count_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(256), 0, stream, d_cw, d_chan, d_hard, n, max_iters, trial);
    return hipGetLastError();
}

}  // namespace ldpc
