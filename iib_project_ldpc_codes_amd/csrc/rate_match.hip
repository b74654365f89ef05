// Rate matching: the channel of a punctured / shortened codeword and the error counts under a count
// mask.  The C ABI's ldpc_channel_rm_dev and ldpc_mc_rm_count_dev (include/ldpc_mi355x.h) launch
// these.  The description is one byte per variable (rate_match_host.cpp packs and validates it):
// bits 0-1 the class (LDPC_RM_TX / _PUNCT / _KNOWN), bit 2 the count mask, the array padded to a
// multiple of four bytes with LDPC_RM_PUNCT, uncounted -- so a dword of it describes the four
// positions 4g .. 4g + 3 and a padding position is neither drawn nor counted.
//
// channel_rm_kernel<VEC>: a thread owns four positions of one trial, as channel_cw_kernel does, and
//   reads their description as one dword.  Where one of them is transmitted it runs
//   channel_cw_kernel's arithmetic (channel_cw.hpp: one copy for both kernels) and keeps the values
//   of the transmitted ones; where none is it draws nothing, no Philox block and no Box-Muller pair.
//   VEC: one 16-byte store of the four LLRs (one dword of the four BEC words) and one dword load of
//   the four codeword bytes; else stores and loads per position.
// rm_count_kernel<KIND, VEC>: one 256-thread workgroup per trial, a thread per description dword.
//   KIND 0: BEC words (channel and decoder output: 2 = erased), 1: LLRs, 2: received bits.  VEC: the
//   four values of each buffer in one load.
#include "channel_cw.hpp"
#include "device_common.hpp"
#include "ldpc_internal.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {
namespace {

constexpr uint32_t kRmClass = 3u, kRmCount = 4u;  // bits of a description byte

template <bool VEC>
__global__ __launch_bounds__(256) void channel_rm_kernel(const uint32_t *__restrict__ desc, int kind, float p, float p2,
                                                         float known, uint64_t seed, uint64_t first_cw, int n, int B,
                                                         const uint8_t *__restrict__ cw, void *out) {
    const int groups = (n + 3) >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)groups * B) return;
    const int b = (int)(idx / groups), g = (int)(idx % groups);
    const uint32_t d = desc[g];
    const size_t o0 = (size_t)b * n + 4 * g;
    uint32_t xs = 0u;  // VEC: the four codeword bytes (n % 4 == 0, cw 4-byte aligned)
    if (VEC && cw) xs = reinterpret_cast<const uint32_t *>(cw)[idx];
    // what a position shows when it is not transmitted: as 32 bits, the BEC word or the LLR's pattern
    uint32_t res[4];
    bool any_tx = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t cls = d >> (8 * i) & kRmClass;
        any_tx |= cls == LDPC_RM_TX;
        bool x = false;
        if (VEC) x = xs >> (8 * i) & 1u;
        else if (cls == LDPC_RM_KNOWN && cw && 4 * g + i < n) x = cw[o0 + i] & 1u;
        if (kind == 0) res[i] = cls == LDPC_RM_KNOWN ? (x ? 1u : 0u) : 2u;
        else res[i] = cls == LDPC_RM_KNOWN ? __float_as_uint(x ? -known : known) : 0u;  // punctured: +0.0f
    }
    if (any_tx) {
        channel_cw_group(
            kind, p, p2, seed, first_cw, n, groups, idx, cw,
            [&](int i, size_t, uint8_t word) {
                if ((d >> (8 * i) & kRmClass) == LDPC_RM_TX) res[i] = word;
            },
            [&](int i, size_t, float llr) {
                if ((d >> (8 * i) & kRmClass) == LDPC_RM_TX) res[i] = __float_as_uint(llr);
            });
    }
    if (VEC) {  // n % 4 == 0: groups = n / 4, the thread's four positions start at element 4 idx
        if (kind == 0) reinterpret_cast<uint32_t *>(out)[idx] = res[0] | res[1] << 8 | res[2] << 16 | res[3] << 24;
        else reinterpret_cast<uint4 *>(out)[idx] = make_uint4(res[0], res[1], res[2], res[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (4 * g + i >= n) break;
            if (kind == 0) static_cast<uint8_t *>(out)[o0 + i] = (uint8_t)res[i];
            else static_cast<uint32_t *>(out)[o0 + i] = res[i];
        }
    }
}

// row[0]: channel errors over the transmitted, counted positions; row[iters]: final errors over the
// counted ones; the entries between them 0 (cw_count_kernel's row).  cw nullptr: the all-zero codeword.
// VEC (n % 4 == 0, every buffer aligned to its load): the four codeword bytes, decisions and channel
// values of a description dword come as one dword (16 bytes of LLRs) each.
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void rm_count_kernel(const uint32_t *__restrict__ desc,
                                                       const uint8_t *__restrict__ cw, const void *__restrict__ chan,
                                                       const uint8_t *__restrict__ dec, int n, int iters,
                                                       int32_t *__restrict__ trial) {
    __shared__ int red[256 / kWave];
    const size_t base = (size_t)blockIdx.x * n;
    const int groups = (n + 3) >> 2;
    int ce = 0, fe = 0;
    for (int g = threadIdx.x; g < groups; g += 256) {
        const uint32_t d = desc[g];
        if (!(d & 0x01010101u * kRmCount)) continue;  // none of the four is counted
        uint32_t xs = 0u, ds = 0u, cs = 0u;  // VEC: bytes 4g .. 4g + 3 of the row
        float4 cf = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (VEC) {
            const size_t q = (base >> 2) + g;
            if (cw) xs = reinterpret_cast<const uint32_t *>(cw)[q];
            ds = reinterpret_cast<const uint32_t *>(dec)[q];
            if (KIND == 1) cf = static_cast<const float4 *>(chan)[q];
            else cs = static_cast<const uint32_t *>(chan)[q];
        }
        const float cfs[4] = {cf.x, cf.y, cf.z, cf.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t by = d >> (8 * i);
            const int v = 4 * g + i;
            if (!(by & kRmCount) || v >= n) continue;  // the padding is uncounted: v < n here anyway
            const bool tx = (by & kRmClass) == LDPC_RM_TX;
            const uint32_t x = VEC ? xs >> (8 * i) & 1u : (cw ? cw[base + v] & 1u : 0u);
            const uint32_t dv = VEC ? ds >> (8 * i) & 0xffu : dec[base + v];
            if (KIND == 0) {
                const uint32_t c = VEC ? cs >> (8 * i) & 0xffu : static_cast<const uint8_t *>(chan)[base + v];
                ce += tx && c == 2;
                fe += dv == 2;
            } else {
                if (tx) {
                    uint32_t y;
                    if (KIND == 1) y = (VEC ? cfs[i] : static_cast<const float *>(chan)[base + v]) < 0.0f ? 1u : 0u;
                    else y = (VEC ? cs >> (8 * i) : static_cast<const uint8_t *>(chan)[base + v]) & 1u;
                    ce += y != x;
                }
                fe += (dv & 1u) != x;
            }
        }
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

template <int KIND>
hipError_t launch_rm_count_kind(bool vec, const uint32_t *desc, const uint8_t *d_cw, const void *d_chan,
                                const uint8_t *d_dec, int n, int B, int max_iters, int32_t *trial, hipStream_t stream) {
    auto kernel = vec ? rm_count_kernel<KIND, true> : rm_count_kernel<KIND, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(256), 0, stream, desc, d_cw, d_chan, d_dec, n, max_iters, trial);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_channel_rm(const uint8_t *d_desc, int channel, float p, float p2, float known_llr, uint64_t seed,
                             uint64_t first_cw, int n, int B, const uint8_t *d_cw, void *d_out, hipStream_t stream) {
    if (B <= 0 || n <= 0) return hipSuccess;
    const size_t total = (size_t)((n + 3) / 4) * (size_t)B;
    const uintptr_t width = channel == 0 ? 3 : 15;  // the store: a dword of BEC words, 16 bytes of LLRs
    const bool vec = n % 4 == 0 && (reinterpret_cast<uintptr_t>(d_out) & width) == 0 &&
                     (reinterpret_cast<uintptr_t>(d_cw) & 3) == 0;
    auto kernel = vec ? channel_rm_kernel<true> : channel_rm_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const uint32_t *>(d_desc), channel, p, p2, known_llr, seed, first_cw, n, B, d_cw,
                       d_out);
    return hipGetLastError();
}

hipError_t launch_rm_count(const uint8_t *d_desc, const uint8_t *d_cw, const void *d_chan, int chan_kind,
                           const uint8_t *d_dec, int n, int B, int max_iters, int32_t *trial, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    const uint32_t *desc = reinterpret_cast<const uint32_t *>(d_desc);
    const auto off = [](const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    const bool vec = n % 4 == 0 && !off(d_cw, 3) && !off(d_dec, 3) && !off(d_chan, chan_kind == 1 ? 15 : 3);
    if (chan_kind == 0) return launch_rm_count_kind<0>(vec, desc, d_cw, d_chan, d_dec, n, B, max_iters, trial, stream);
    if (chan_kind == 1) return launch_rm_count_kind<1>(vec, desc, d_cw, d_chan, d_dec, n, B, max_iters, trial, stream);
    return launch_rm_count_kind<2>(vec, desc, d_cw, d_chan, d_dec, n, B, max_iters, trial, stream);
}

}  // namespace ldpc
