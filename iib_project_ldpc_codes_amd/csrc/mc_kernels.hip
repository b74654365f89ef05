// Stand-alone channel and the Monte-Carlo statistics kernels (stop rule, counter reduction).
//
// Reference behaviour restated here:
//   channels.py:24-26 new_transmit -> channel_kernel / chan_* (same law, Philox)
//   parallel_simulator.py:198-244  -> mc_* (per-trial statistics + stop rule)
#include <rocrand/rocrand_kernel.h>

#include "device_common.hpp"
#include "ldpc_internal.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {
namespace {

// ===========================================================================
// 3. Stand-alone channel (rocRAND philox4x32_10 device API)
// ===========================================================================
__global__ __launch_bounds__(256) void channel_kernel(int kind, float p, float p2, uint64_t seed,
                                                      uint64_t first_cw, int n, int B, void *out) {
    const int groups = (n + 3) >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)groups * B) return;
    const int b = (int)(idx / groups), g = (int)(idx % groups);
    rocrand_state_philox4x32_10 st;
    rocrand_init(seed, first_cw + (uint64_t)b, 4ull * (uint64_t)g, &st);
    const uint4 r = rocrand4(&st);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
    float val[4];
    if (kind == 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float ua = u01(w[2 * h]), ub = u01(w[2 * h + 1]);
            const float rad = sqrtf(-2.0f * logf(ua));
            const float ang = 6.28318530717958647692f * ub;
            val[2 * h] = (1.0f + p * (rad * cosf(ang))) * p2;
            val[2 * h + 1] = (1.0f + p * (rad * sinf(ang))) * p2;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = 4 * g + i;
        if (v >= n) break;
        const size_t o = (size_t)b * n + v;
        const float u = u01(w[i]);
        if (kind == 0) static_cast<uint8_t *>(out)[o] = u < p ? 2 : 0;
        else if (kind == 1) static_cast<float *>(out)[o] = u < p ? -p2 : p2;
        else static_cast<float *>(out)[o] = val[i];
    }
}

// ===========================================================================
// 4. Monte-Carlo statistics: sequential stop rule + counter reduction
// ===========================================================================
// Trial b is a frame error when its final count f satisfies f > X && f != 0
// (parallel_simulator_expurgated.py:238-243; X = -1 gives parallel_simulator.py:227-231).
__global__ __launch_bounds__(1024) void mc_cutoff_kernel(const int32_t *trial, int B, int iters, int X,
                                                         int64_t stop, const int64_t *counters,
                                                         int32_t *cutoff) {
    __shared__ int cnt[1024];
    __shared__ int res;
    const int tid = threadIdx.x;
    if (stop <= 0) {
        if (tid == 0) *cutoff = B;
        return;
    }
    const int64_t remaining = stop - counters[1];
    if (remaining <= 0) {
        if (tid == 0) *cutoff = 0;
        return;
    }
    const int chunk = (B + 1023) / 1024;
    const int b0 = tid * chunk, b1 = min(B, b0 + chunk);
    int c = 0;
    for (int b = b0; b < b1; ++b) {
        const int f = trial[(size_t)b * (iters + 1) + iters];
        c += (f > X && f != 0);
    }
    cnt[tid] = c;
    if (tid == 0) res = B;
    __syncthreads();
    if (tid == 0) {  // exclusive scan (1024 adds)
        int acc = 0;
        for (int i = 0; i < 1024; ++i) {
            const int t = cnt[i];
            cnt[i] = acc;
            acc += t;
        }
    }
    __syncthreads();
    const int64_t before = cnt[tid];
    if (before < remaining && before + c >= remaining) {
        int64_t acc = before;
        for (int b = b0; b < b1; ++b) {
            const int f = trial[(size_t)b * (iters + 1) + iters];
            acc += (f > X && f != 0);
            if (acc >= remaining) {
                res = b + 1;
                break;
            }
        }
    }
    __syncthreads();
    if (tid == 0) *cutoff = res;
}

__global__ __launch_bounds__(256) void mc_reduce_kernel(const int32_t *trial, const int32_t *its, int B,
                                                        int iters, int X, const int32_t *cutoff_p,
                                                        int64_t *counters) {
    __shared__ long long red[4][256 / kWave];
    const int tid = threadIdx.x;
    const int cutoff = min(B, *cutoff_p);
    const int per = (B + gridDim.x - 1) / gridDim.x;
    const int b0 = blockIdx.x * per, b1 = min(cutoff, b0 + per);
    if (b0 >= b1) return;
    // error curve columns, coalesced over t
    for (int t = tid; t <= iters; t += 256) {
        long long s = 0;
        for (int b = b0; b < b1; ++b) {
            const int32_t *row = trial + (size_t)b * (iters + 1);
            if (row[iters] > X) s += row[t];
        }
        if (s) atomicAdd(reinterpret_cast<unsigned long long *>(counters + LDPC_MC_NCOUNT + t),
                         (unsigned long long)s);
    }
    long long fr = 0, bits = 0, itn = 0;
    for (int b = b0 + tid; b < b1; b += 256) {
        const int f = trial[(size_t)b * (iters + 1) + iters];
        if (f > X) {
            fr += (f != 0);
            bits += f;
        }
        itn += its ? its[b] : 0;
    }
    long long v[3] = {fr, bits, itn};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        long long x = v[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
        if ((tid & 63) == 0) red[q][tid / kWave] = x;
    }
    __syncthreads();
    if (tid == 0) {
        long long s[3] = {0, 0, 0};
        for (int q = 0; q < 3; ++q)
            for (int w = 0; w < 256 / kWave; ++w) s[q] += red[q][w];
        unsigned long long *c = reinterpret_cast<unsigned long long *>(counters);
        atomicAdd(c + 0, (unsigned long long)(b1 - b0));
        atomicAdd(c + 1, (unsigned long long)s[0]);
        atomicAdd(c + 2, (unsigned long long)s[1]);
        atomicAdd(c + 3, (unsigned long long)s[2]);
    }
}

}  // namespace

hipError_t launch_channel(int channel, float p, float p2, uint64_t seed, uint64_t first_cw, int n, int B,
                          void *d_out, hipStream_t stream) {
    if (B <= 0 || n <= 0) return hipSuccess;
    const size_t total = (size_t)((n + 3) / 4) * (size_t)B;
    const unsigned grid = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(channel_kernel, dim3(grid), dim3(256), 0, stream, channel, p, p2, seed, first_cw, n, B,
                       d_out);
    return hipGetLastError();
}

hipError_t launch_mc_reduce(const int32_t *trial, const int32_t *trial_its, int B, int max_iters,
                            int expurgation, int64_t stop_frame_errors, int64_t *d_counters,
                            int32_t *d_cutoff, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(mc_cutoff_kernel, dim3(1), dim3(1024), 0, stream, trial, B, max_iters, expurgation,
                       stop_frame_errors, d_counters, d_cutoff);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_mc_reduce_cut(trial, trial_its, B, max_iters, expurgation, d_cutoff, d_counters, stream);
}

hipError_t launch_mc_reduce_cut(const int32_t *trial, const int32_t *trial_its, int B, int max_iters, int expurgation,
                                const int32_t *d_cutoff, int64_t *d_counters, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    const int blocks = B < 1024 ? (B + 63) / 64 : 256;
    hipLaunchKernelGGL(mc_reduce_kernel, dim3(blocks), dim3(256), 0, stream, trial, trial_its, B, max_iters,
                       expurgation, d_cutoff, d_counters);
    return hipGetLastError();
}

}  // namespace ldpc
