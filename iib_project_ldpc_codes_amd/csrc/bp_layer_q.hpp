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

}  // namespace
}  // namespace ldpc
