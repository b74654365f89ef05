// The channel of a transmitted codeword, for the four positions 4g .. 4g + 3 of one trial: the one
// copy of the arithmetic that channel_cw_kernel (encode.hip) and channel_rm_kernel (rate_match.hip)
// both run, so that a transmitted position of a rate-matched word is ldpc_channel_cw_dev's value
// bit for bit.  channel_kernel (mc_kernels.hip) word for word, then the reflection where the
// codeword bit is 1.
#pragma once
#include <rocrand/rocrand_kernel.h>

#include "device_common.hpp"

namespace ldpc {
namespace {

// Thread idx of the launch owns positions 4g .. 4g + 3 (those below n) of row b = idx / groups, trial
// first_cw + b, g = idx % groups, groups = ceil(n / 4).  Position i of them, at offset o = b n + 4g + i,
// goes to bec(i, o, word) on the BEC (kind 0: the erasure 2, otherwise the codeword bit) and to
// soft(i, o, llr) on the BSC (kind 1) and the BI-AWGN channel (the LLR, negated where the codeword
// bit is 1); cw nullptr: the all-zero codeword.
template <typename Bec, typename Soft>
__device__ __forceinline__ void channel_cw_group(int kind, float p, float p2, uint64_t seed, uint64_t first_cw, int n,
                                                 int groups, size_t idx, const uint8_t *__restrict__ cw, Bec bec,
                                                 Soft soft) {
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
        const bool x = cw && (cw[o] & 1u);
        if (kind == 0) {
            bec(i, o, u < p ? 2 : (x ? 1 : 0));
        } else {
            const float llr = kind == 1 ? (u < p ? -p2 : p2) : val[i];
            soft(i, o, x ? -llr : llr);
        }
    }
}

}  // namespace
}  // namespace ldpc
