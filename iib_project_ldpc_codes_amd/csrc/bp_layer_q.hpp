// What the fixed-point layered min-sum kernels share (bp_layer_q.hip on a layer schedule's tables,
// bp_qc_q.hip on a quasi-cyclic code's block rows): the channel quantiser and the step of one check
// on registers, from its record and posteriors in LDS back to them.  Semantics:
// include/ldpc_mi355x.h, ldpc_bp_layered_q_decode_batch_dev.
//
// The record of a check holds what its messages R are rebuilt from: the two magnitudes f(m1) and
// f(m2), the index i1 of the first minimum and one sign bit per edge --
//   check degree <= 16: one word   f(m1) | f(m2) << 6 | i1 << 12 | signs << 16
//   check degree <= 32: two words  f(m1) | f(m2) << 6 | i1 << 12,  signs
// (magnitudes <= Q <= 63).
#pragma once
#include "bp_device.hpp"
#include "ldpc_mi355x.h"  // LDPC_RM_*

namespace ldpc {
namespace {

typedef __attribute__((address_space(3))) signed char lds_i8;
typedef __attribute__((address_space(3))) uint32_t lds_u32;

// The channel quantiser: rint_half_even(clamp(l * scale, -Q, +Q)), NaN -> 0 (one fp32 product;
// the library is built without contraction)
__device__ __forceinline__ int quantise(float l, float scale, int Q) {
    const float t = l * scale;
    if (t != t) return 0;
    return (int)__builtin_rintf(fminf(fmaxf(t, (float)-Q), (float)Q));
}

// The step of one check, over the kernel's own P, rec and quantiser scalars (held by reference,
// as a lambda of the kernel would): step(c, d, v) is the check with record c (RW = 1 or 2 words
// each), degree d > 0 and variables v (an entry past d: any byte of P, its value is not used).
// Every load before the first use.
template <int MAXDC>
struct LayerQStep {
    lds_i8 *const &P;
    lds_u32 *const &rec;
    const int &Q, &Pmax, &norm8, &offset;
    __device__ void operator()(int c, int d, const int (&v)[MAXDC]) const {
        constexpr int RW = MAXDC <= 16 ? 1 : 2;            // words of a record
        constexpr uint32_t IMASK = MAXDC <= 16 ? 15 : 31;  // the index field
        auto f = [&](int mag) { return max(((mag * norm8) >> 3) - offset, 0); };
        int x[MAXDC];
#pragma unroll
        for (int j = 0; j < MAXDC; ++j) x[j] = P[v[j]];  // an absent edge reads some byte
        const uint32_t w0 = rec[c * RW];
        const uint32_t sg = RW == 2 ? rec[c * RW + 1] : w0 >> 16;
        const int f1 = w0 & 63, f2 = (w0 >> 6) & 63, i1 = (w0 >> 12) & IMASK;
        // x_j = P - R_j, R_j rebuilt from the record; the min1 / min2 / index scan (an absent
        // edge enters as magnitude Q, positive: it lowers neither minimum and is never first)
        int a_[MAXDC];
        uint32_t neg = 0;
#pragma unroll
        for (int j = 0; j < MAXDC; ++j) {
            const int mag = j == i1 ? f2 : f1;
            x[j] -= (sg >> j) & 1 ? -mag : mag;
            const bool has = j < d;
            a_[j] = has ? min(abs(x[j]), Q) : Q;
            neg |= (uint32_t)(has && x[j] < 0) << j;
        }
        int m1 = a_[0], m2 = Q, k1 = 0;
#pragma unroll
        for (int j = 1; j < MAXDC; ++j) {
            const bool lt = a_[j] < m1;
            m2 = lt ? m1 : min(m2, a_[j]);
            k1 = lt ? j : k1;
            m1 = lt ? a_[j] : m1;
        }
        const int g1 = f(m1), g2 = f(m2);
        const uint32_t par = __builtin_popcount(neg) & 1;
        // r_j is negative iff parity ^ s_j, and |r_j| > 0
        uint32_t rs = (par ? ~neg : neg) & (d >= 32 ? 0xFFFFFFFFu : (1u << d) - 1u);
        if (g1 == 0) rs &= 1u << k1;
        if (g2 == 0) rs &= ~(1u << k1);
#pragma unroll
        for (int j = 0; j < MAXDC; ++j)
            if (j < d) {
                const int mag = j == k1 ? g2 : g1;
                const int r = (rs >> j) & 1 ? -mag : mag;
                P[v[j]] = (signed char)min(max(x[j] + r, -Pmax), Pmax);
            }
        const uint32_t head = (uint32_t)g1 | (uint32_t)g2 << 6 | (uint32_t)k1 << 12;
        if constexpr (RW == 2) {
            rec[c * RW] = head;
            rec[c * RW + 1] = rs;
        } else {
            rec[c] = head | rs << 16;
        }
    }
};

// ---- The codeword mode (include/ldpc_mi355x.h, ldpc_mc_layered_q_cw_batch_dev): the channel of a
// transmitted, rate-matched codeword drawn into P, and the count of every iteration against it.
// After the records the block holds one bit per variable of the codeword: word w >> 3, nibble w & 7
// of the plane belongs to word w of P, so the count stays one pass over P's words.  The count mask
// is not kept in LDS: the count re-reads the description's dword w (the batch's, 4 ceil(n / 4) bytes,
// coalesced and cache-resident), whose count bits shift onto the sign bits of P's bytes.
constexpr uint32_t kCwClass = 3u, kCwCount = 4u;  // bits of a description byte (rate_match.hip)

// The kernels' optional last argument: itself, or nothing read
__device__ __forceinline__ CwArgs cw_args() { return CwArgs{}; }
__device__ __forceinline__ CwArgs cw_args(const CwArgs &c) { return c; }

// bit i of a nibble -> the sign bit of byte i
__device__ __forceinline__ uint32_t nibble_to_signs(uint32_t nib) { return ((nib * 0x00204081u) & 0x01010101u) << 7; }
// bit 0 of byte i -> bit i of a nibble
__device__ __forceinline__ uint32_t lsbs_to_nibble(uint32_t w) { return ((w & 0x01010101u) * 0x10204080u) >> 28; }

// Nibble g of a plane from the thread that owns group g.  The eight lanes g & ~7 .. g | 7 of a wave
// call it together (g & 7 is the lane's), fold their nibbles within the row and lane 0 of them stores.
__device__ __forceinline__ void plane_store(lds_u32 *plane, int g, uint32_t nib) {
    int v = (int)(nib << (4 * (g & 7)));
    v |= __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    v |= __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    v |= __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);  // row_half_mirror: the other quad
    if ((g & 7) == 0) plane[g >> 3] = (uint32_t)v;
}

// The description dword of group g: the caller's, or every position below n transmitted and
// counted; a position from n on is punctured and uncounted either way.
__device__ __forceinline__ uint32_t cw_desc(const CwArgs &c, int g, int n) {
    const int left = n - 4 * g;
    if (left <= 0) return 0x01010101u * LDPC_RM_PUNCT;
    if (c.desc) return c.desc[g];
    const uint32_t low = left >= 4 ? 0xFFFFFFFFu : (1u << (8 * left)) - 1u;
    return (0x01010101u * (LDPC_RM_TX | kCwCount) & low) | (0x01010101u * LDPC_RM_PUNCT & ~low);
}

// Row b of the batch (trial `trial`) into P and the codeword plane xp, by groups of four positions:
// one Philox block per group with a transmitted position (channel_cw_group's arithmetic, on
// chan_block's block), the three rules of a description byte, the reflection, the quantiser, one
// dword store of the four bytes of P (the padding bytes 0).  Returns the thread's part of row[0]:
// the transmitted, counted positions whose float's sign differs from the codeword bit -- or, with
// no iteration to come, the counted positions whose quantised value's does.
template <int T>
__device__ __forceinline__ int cw_stage(const LayerQArgs &a, const CwArgs &c, int b, uint64_t trial, lds_u32 *Pw,
                                        lds_u32 *xp) {
    const int n = a.n, n4 = (n + 3) >> 2;
    const size_t base = (size_t)b * n;
    int err = 0;
    for (int g = threadIdx.x; g < 8 * ((n + 31) >> 5); g += T) {  // whole plane words: see plane_store
        const uint32_t d = cw_desc(c, g, n);
        uint32_t xs = 0u;
        if (c.cw && g < n4) {
            if (c.vec) {
                xs = reinterpret_cast<const uint32_t *>(c.cw)[(base >> 2) + g];
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * g + i < n) xs |= (uint32_t)c.cw[base + 4 * g + i] << (8 * i);
            }
        }
        bool tx[4], any_tx = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            tx[i] = (d >> (8 * i) & kCwClass) == LDPC_RM_TX;
            any_tx |= tx[i];
        }
        float val[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (any_tx) {
            const uint4 r = chan_block(a.ch, trial, g);
            const uint32_t w[4] = {r.x, r.y, r.z, r.w};
            if (a.ch.kind == 1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) val[i] = u01(w[i]) < a.ch.p ? -a.ch.p2 : a.ch.p2;
            } else {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float ua = u01(w[2 * h]), ub = u01(w[2 * h + 1]);
                    const float rad = sqrtf(-2.0f * logf(ua));
                    const float ang = 6.28318530717958647692f * ub;
                    val[2 * h] = (1.0f + a.ch.p * (rad * cosf(ang))) * a.ch.p2;
                    val[2 * h + 1] = (1.0f + a.ch.p * (rad * sinf(ang))) * a.ch.p2;
                }
            }
        }
        uint32_t pw = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t by = d >> (8 * i);
            const bool x = xs >> (8 * i) & 1u, counted = by & kCwCount;
            float llr = 0.0f;  // punctured: +0.0f
            if (tx[i]) llr = x ? -val[i] : val[i];
            else if ((by & kCwClass) == LDPC_RM_KNOWN) llr = x ? -c.known : c.known;
            const int q = quantise(llr, a.scale, a.Q);
            pw |= (uint32_t)(q & 0xff) << (8 * i);
            if (a.max_iters == 0) err += counted && (q < 0) != x;
            else err += tx[i] && counted && (llr < 0.0f) != x;
        }
        if (g < n4) Pw[g] = pw;
        plane_store(xp, g, lsbs_to_nibble(xs));
    }
    return err;
}

// The thread's part of #{v : count = 1, [P_v < 0] != x_v}, over P's words; desc nullptr: every
// position counts (the padding bytes of P and of the plane are 0).  Four description dwords are
// loaded ahead of the words they mask.
template <int T>
__device__ __forceinline__ int cw_count(const lds_u32 *Pw, const lds_u32 *xp, const uint32_t *__restrict__ desc, int n4) {
    auto wrong = [&](int w) { return (Pw[w] ^ nibble_to_signs(xp[w >> 3] >> (4 * (w & 7)) & 15u)) & 0x80808080u; };
    int errs = 0;
    if (!desc) {
        for (int w = threadIdx.x; w < n4; w += T) errs += __builtin_popcount(wrong(w));
        return errs;
    }
    for (int w0 = threadIdx.x; w0 < n4; w0 += 4 * T) {
        uint32_t d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = w0 + k * T < n4 ? desc[w0 + k * T] : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (w0 + k * T < n4) errs += __builtin_popcount(wrong(w0 + k * T) & d[k] << 5);  // kCwCount -> the sign bit
    }
    return errs;
}

}  // namespace
}  // namespace ldpc
