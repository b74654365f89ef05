// Device helpers shared by the soft-decoding kernels (bp_lds.hip, bp_loc.hpp, bp_irr.hip,
// bp_generic.hip): message domains, wire / ratio helpers, the check-node updates.
#pragma once
#include "kernel_args.hpp"

namespace ldpc {
namespace {

// ===========================================================================
// 2. Soft flooding BP (no reference counterpart; oracle_bp_decode defines it)
// ===========================================================================
// Sum-product runs in the log2 domain (messages are LLR / ln 2) and in the
// ratio form of oracle check_update_spa: e_i = 2^-min(|x_i|, 23) is one
// v_exp_f32, the exclusive product of tanh(x_i/2) = a_i / b_i (a_i = sign*(1-e_i),
// b_i = 1+e_i) is N_j / D_j from prefix/suffix products, and 2 atanh(N/D) / ln 2 =
// log2((D+N) / (D-N)) is one v_rcp_f32 + one v_log_f32 -- three transcendentals
// per edge.  Channel LLRs are scaled by log2(e) in, posteriors by ln 2 out.
template <int ALGO> struct Domain {
    static constexpr float in = ALGO == 0 ? 1.44269504088896341f : 1.0f;   // LLR -> message units
    static constexpr float out = ALGO == 0 ? 0.693147180559945309f : 1.0f; // message units -> LLR
};
// Channel LLR -> message.  Min-sum: l + 0 turns a -0 LLR into +0 (every other value is
// unchanged), so no min-sum message is ever -0 (sums and differences of non-(-0) values
// are not -0 in round-to-nearest) and the sign BIT of every check input equals the
// oracle's (x < 0) -- which lets check_update_ms6 form signs with bit operations.
template <int ALGO> __device__ __forceinline__ float to_msg(float l) {
    if constexpr (ALGO == 0) return l * Domain<0>::in;
    else return l + 0.0f;
}

// Sum-product check rule in ratio form, restated by oracle check_update_spa: for an
// input message x (log2 units here) tanh(x/2) = (R - 1) / (R + 1) with the ratio
// R = 2^x, |x| clamped to 23 (R in [2^-23, 2^23]); the exclusive products of the
// (R - 1) and (R + 1) terms give the output 2 atanh(N_j / D_j) / ln 2 =
// log2((D_j + N_j) / (D_j - N_j)) -- formed without cancellation from elementary
// symmetric polynomials of the R (check_update_spa_pair_rwire).
//
// v->c message "on the wire" of the LDS kernels: sum-product sends the clamped ratio R
// itself (the check rule's outputs (D + N) / (D - N) are invariant to a positive scale of
// each input's (R - 1, R + 1) pair, so no reciprocal per edge in the variable phase;
// magnitudes stay below 2^23 + 1, so the exclusive products of 5 inputs stay below
// 2^116); min-sum sends x itself.
template <int ALGO>
__device__ __forceinline__ float v2c_rwire(float x) {
    if (ALGO == 0) return __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(x, -23.0f, 23.0f));
    return x;
}
// an extrinsic ratio R on the wire: clamped to [2^-23, 2^23]
__device__ __forceinline__ float ratio_wire(float R) { return __builtin_amdgcn_fmed3f(R, 0x1p-23f, 0x1p23f); }
__device__ __forceinline__ float2 ratio_wire2(float2 R) {
    return make_float2(__builtin_amdgcn_fmed3f(R.x, 0x1p-23f, 0x1p23f), __builtin_amdgcn_fmed3f(R.y, 0x1p-23f, 0x1p23f));
}

// Inline-asm helpers (v_bitop3_b32, the VCC select): the compiler's hazard
// recognizer does not look inside inline asm, so their operands must not be fresh
// transcendental (v_exp / v_log / v_rcp) results -- every use below takes LDS loads, min /
// med3 / mul / bfe results or values from an earlier phase.
// v_bitop3_b32 (gfx950) with truth table T over (S0, S1, S2) = (0xF0, 0xCC, 0xAA)
// (check_update_ms6's sign stamps stay in asm: through the builtin the fixed-count min-sum
// decode measured 1.3 % slower, profiles/r05_ab_bitop3_builtin.txt)
template <int T>
__device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:%4" : "=v"(r) : "v"(a), "v"(b), "v"(c), "n"(T));
    return r;
}
// a ^ b ^ c in one instruction (gfx950 has no v_xor3_b32: v_bitop3_b32 with table 0x96).
// Through the builtin, as bfi_u32: the hazard recognizer sees the instruction and inserts no
// conservative s_nop around it (early stop +0.9 %, min-sum Monte-Carlo +1.2 %,
// profiles/r05_ab_xor3_bfi_builtin.txt)
__device__ __forceinline__ uint32_t xor3u(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
// |x| == m ? t : f as v_cmp (into VCC) + v_cndmask: the compiler would otherwise hold one
// SGPR-pair mask per output of a check pair at once and spill SGPRs
__device__ __forceinline__ uint32_t sel_abs_eq(float x, float m, uint32_t t, uint32_t f) {
    uint32_t r;
    asm("v_cmp_eq_f32_e64 vcc, |%1|, %2\n\tv_cndmask_b32 %0, %4, %3, vcc" : "=v"(r) : "v"(x), "v"(m), "v"(t), "v"(f) : "vcc");
    return r;
}
// (m & a) | (~m & b): one v_bitop3_b32 (table 0xCA), through the builtin (see xor3u)
__device__ __forceinline__ uint32_t bfi_u32(uint32_t m, uint32_t a, uint32_t b) {
    return __builtin_amdgcn_bitop3_b32(m, a, b, 0xCA);
}
// (r & ~1) | (d & 1): one v_bfi_b32
// (plain C: the compiler emits one v_and_or_b32 / v_bfi_b32 and, unlike for inline asm, inserts
// the wait state gfx950 needs when an operand is a fresh transcendental result -- an asm
// v_bfi_b32 right after the v_exp_f32 of the initial message read a stale register)
__device__ __forceinline__ uint32_t bfi_lsb(uint32_t r, uint32_t d) { return (r & ~1u) | (d & 1u); }

// a * b + c per lane as one v_pk_fma_f32 (the SLP vectoriser packs only some)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 pk_fma(float2 a, float2 b, float2 c) {
    const f32x2 r = __builtin_elementwise_fma(f32x2{a.x, a.y}, f32x2{b.x, b.y}, f32x2{c.x, c.y});
    return make_float2(r.x, r.y);
}

// Check-node update over D messages in registers; entries i >= d are padding (+inf
// for min-sum; skipped by sum-product).  Min-sum is bit-exact with oracle
// check_update_ms; sum-product agrees with the oracle's exact rule to the stated
// tolerance (tests/test_gpu_fallback.py for D > 6).
template <int ALGO, int D, bool WIRE = false>
__device__ __forceinline__ void check_update(float (&x)[D], float alpha, int d = D) {
    if constexpr (ALGO == 0 && D > 6) {
        // The same elementary-symmetric form, rescaled per input: e_k of the form below reaches
        // 2^(23 k), so six saturated inputs overflow fp32 (degree >= 7: inf * 0 = NaN).  The
        // (E, O) recurrence is homogeneous in each input's pair (1, R), so an input with R > 1
        // enters as (1 / R, 1): with r = 2^-|x| <= 1,
        //   R > 1:   (E, O) <- (r E + O, r O + E)        otherwise:   (E, O) <- (E + r O, O + r E).
        // E + O = prod (1 + r_i) <= 2^31 and min(E, O) >= sum r_i >= 2^-23 at 32 inputs, all terms
        // positive; the output ratio num / den is unchanged (oracle algo 3 restates it).
        float r[D];
        bool big[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            if constexpr (WIRE) {
                big[i] = x[i] > 1.0f;
                r[i] = big[i] ? __builtin_amdgcn_rcpf(x[i]) : x[i];
            } else {
                big[i] = x[i] > 0.0f;
                r[i] = __builtin_amdgcn_exp2f(-fminf(fabsf(x[i]), 23.0f));
            }
        }
        auto grow = [](float2 s, float ri, bool bi) {  // (E, O) of the set plus one input
            const float2 t = make_float2(s.y, s.x);
            return pk_fma(make_float2(ri, ri), bi ? s : t, bi ? t : s);
        };
        float2 pre[D];  // scaled (E, O) of inputs {0 .. i-1}
        pre[0] = make_float2(1.0f, 0.0f);
#pragma unroll
        for (int i = 1; i < D; ++i) pre[i] = i - 1 < d ? grow(pre[i - 1], r[i - 1], big[i - 1]) : pre[i - 1];
        const bool odd = (d - 1) & 1;
        float2 suf = make_float2(1.0f, 0.0f);  // scaled (E, O) of inputs {j+1 .. d-1}
#pragma unroll
        for (int j = D - 1; j >= 0; --j) {
            if (j < d) {
                const float E = fmaf(pre[j].x, suf.x, pre[j].y * suf.y), O = fmaf(pre[j].x, suf.y, pre[j].y * suf.x);
                const float num = odd ? O : E, den = odd ? E : O;
                const float2 ns = grow(suf, r[j], big[j]);
                x[j] = __builtin_amdgcn_logf(num * __builtin_amdgcn_rcpf(den));
                suf = ns;
            }
        }
    } else if (ALGO == 0) {
        // elementary-symmetric form (check_update_spa_pair_rwire) on the d inputs' ratios
        // R = 2^x (WIRE: the ratios themselves), outputs log2 of the exclusive ratio; (E, O)
        // sums in float2 so both chains are packed ops.  Entries i >= d are skipped.
        // D <= 6 only: five inputs' e_k stay below 2^118.
        float R[D];
#pragma unroll
        for (int i = 0; i < D; ++i)
            R[i] = WIRE ? x[i] : __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(x[i], -23.0f, 23.0f));
        float2 pre[D];  // (E, O) of inputs {0 .. i-1}
        pre[0] = make_float2(1.0f, 0.0f);
#pragma unroll
        for (int i = 1; i < D; ++i) {
            const float2 nx = pk_fma(make_float2(R[i - 1], R[i - 1]), make_float2(pre[i - 1].y, pre[i - 1].x), pre[i - 1]);
            pre[i] = i - 1 < d ? nx : pre[i - 1];
        }
        const bool odd = (d - 1) & 1;
        float2 suf = make_float2(1.0f, 0.0f);  // (E, O) of inputs {j+1 .. d-1}
#pragma unroll
        for (int j = D - 1; j >= 0; --j) {
            if (j < d) {
                const float E = fmaf(pre[j].x, suf.x, pre[j].y * suf.y), O = fmaf(pre[j].x, suf.y, pre[j].y * suf.x);
                const float num = odd ? O : E, den = odd ? E : O;
                const float2 ns = pk_fma(make_float2(R[j], R[j]), make_float2(suf.y, suf.x), suf);
                x[j] = __builtin_amdgcn_logf(num * __builtin_amdgcn_rcpf(den));
                suf = ns;
            }
        }
    } else {
        // branch-free: m1 = running min, m2 = running second smallest (with
        // multiplicity) = med3(m1, m2, a); an edge whose magnitude equals m1 gets
        // m2 (with a tie m2 == m1: the same values as oracle check_update_ms'
        // "first minimum gets m2")
        float m1 = __builtin_inff(), m2 = __builtin_inff();
        bool neg = false;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const float a = fabsf(x[i]);
            neg ^= (x[i] < 0.0f);
            m2 = __builtin_amdgcn_fmed3f(m1, m2, a);
            m1 = fminf(m1, a);
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const float mag = alpha * (fabsf(x[i]) == m1 ? m2 : m1);
            x[i] = (neg ^ (x[i] < 0.0f)) ? -mag : mag;
        }
    }
}

// Normalized min-sum update of one degree-6 check, branch-free: the two smallest
// magnitudes (with multiplicity) from two triples -- m1 = min of the triple minima,
// m2 = min(max of the triple minima, both triple medians) -- via v_min3 / v_med3.
// An edge whose magnitude equals m1 gets m2 (with a tie m2 == m1, so this equals
// oracle check_update_ms' "index of the first minimum gets m2"); signs as there.
__device__ __forceinline__ void check_update_ms6(float (&x)[6], float alpha) {
    float ax[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) ax[i] = fabsf(x[i]);
    const float mn1 = fminf(fminf(ax[0], ax[1]), ax[2]), md1 = __builtin_amdgcn_fmed3f(ax[0], ax[1], ax[2]);
    const float mn2 = fminf(fminf(ax[3], ax[4]), ax[5]), md2 = __builtin_amdgcn_fmed3f(ax[3], ax[4], ax[5]);
    const float m1 = fminf(mn1, mn2), m2 = fminf(fminf(fmaxf(mn1, mn2), md1), md2);
    float am1 = alpha * m1, am2 = alpha * m2;
    // keep the two products: otherwise select(alpha*m2, alpha*m1) is folded into
    // alpha*select(m2, m1), one multiply per edge instead of two per check
    asm volatile("" : "+v"(am1), "+v"(am2));
    // signs as bits (no input is -0, see to_msg, so the sign bit is the oracle's x < 0):
    // S = XOR of the six sign bits, stamped onto both scaled minima once per check; each
    // output is then the selected minimum XOR its own input's sign bit -- v_cmp, v_cndmask
    // and one v_bitop3 / v_and + v_xor per output, no scalar mask arithmetic
    const uint32_t S = xor3u(xor3u(__float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2])),
                             __float_as_uint(x[3]), __float_as_uint(x[4])) ^ __float_as_uint(x[5]);
    const uint32_t M = 0x80000000u;
    const uint32_t s1 = bitop3<0xF8>(__float_as_uint(am1), S, M), s2 = bitop3<0xF8>(__float_as_uint(am2), S, M);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const uint32_t mag = sel_abs_eq(x[i], m1, s2, s1);  // a | (b & M), then a ^ (b & M)
        x[i] = __uint_as_float(bitop3<0x78>(mag, __float_as_uint(x[i]), M));
    }
}


// Sum-product update of a PAIR of checks held as float2 lanes (.x = check 2q, .y = check
// 2q + 1), every product one packed op for both checks.  The inputs are the clamped
// ratios R_i = e^{x_i} (ratio_wire), and tanh(x_i/2) = (R_i - 1) / (R_i + 1).  With
// D_j = prod_{i != j} (R_i + 1) and N_j = prod_{i != j} (R_i - 1), the output ratio
// (D_j + N_j) / (D_j - N_j) is, expanding both products in the elementary symmetric
// polynomials e_k of the d - 1 inputs i != j, O_j / E_j for d - 1 odd (E_j / O_j for
// d - 1 even), where E = sum_{k even} e_k and O = sum_{k odd} e_k.  Every term is
// positive, so there is no cancellation anywhere (the difference D - N of the ratio
// form loses ~d ulps x e^|c| near saturation): each output is good to ~10 fp32 ulps.
// (E, O) of a set grows by one input R as (E + R O, O + R E) -- two fused multiply-adds,
// the cost of the ratio form's two product chains -- and two disjoint sets combine as
// (E_a E_b + O_a O_b, E_a O_b + O_a E_b).  Magnitudes: E >= 1, O >= sum R >= 2^-23,
// e_k < 2^(23 k + 3) <= 2^118 for the 5 inputs of a degree-6 check.
// INVX: the .x check has one input less, padded with R = 0 (E, O unchanged, but the
// exclusive sets count one more input), so its outputs take the other parity's ratio.
template <int D, bool INVX = false>
__device__ __forceinline__ void check_update_spa_pair_rwire(float2 (&R)[D]) {
    const float2 one = make_float2(1.0f, 1.0f);
    auto ratio = [](float2 E, float2 O) {
        constexpr bool odd = (D - 1) % 2 == 1;
        if constexpr (INVX) {
            return odd ? make_float2(E.x * __builtin_amdgcn_rcpf(O.x), O.y * __builtin_amdgcn_rcpf(E.y))
                       : make_float2(O.x * __builtin_amdgcn_rcpf(E.x), E.y * __builtin_amdgcn_rcpf(O.y));
        }
        if constexpr (odd) return O * make_float2(__builtin_amdgcn_rcpf(E.x), __builtin_amdgcn_rcpf(E.y));
        else return E * make_float2(__builtin_amdgcn_rcpf(O.x), __builtin_amdgcn_rcpf(O.y));
    };
    float2 pE[D], pO[D];  // prefix sets {0 .. i-1}
    pE[1] = one;
    pO[1] = R[0];
#pragma unroll
    for (int i = 2; i < D; ++i) {
        pE[i] = pk_fma(R[i - 1], pO[i - 1], pE[i - 1]);
        pO[i] = pk_fma(R[i - 1], pE[i - 1], pO[i - 1]);
    }
    float2 sE = one, sO = R[D - 1];  // suffix set {i+1 .. D-1}
    R[D - 1] = ratio(pE[D - 1], pO[D - 1]);
#pragma unroll
    for (int i = D - 2; i >= 1; --i) {
        const float2 E = pk_fma(pE[i], sE, pO[i] * sO);
        const float2 O = pk_fma(pE[i], sO, pO[i] * sE);
        const float2 nE = pk_fma(R[i], sO, sE);
        const float2 nO = pk_fma(R[i], sE, sO);
        R[i] = ratio(E, O);
        sE = nE;
        sO = nO;
    }
    R[0] = ratio(sE, sO);
}

// Byte address (x4) of the low / high 16-bit LDS position packed in p: one SDWA
// shift instead of an extract and a shift-add.  volatile: re-evaluated every
// iteration, so the compiler cannot hoist VPT*DV unpacked addresses out of the
// decode loop (they would not fit the VGPR budget).
typedef __attribute__((address_space(3))) float lds_f32;  // LDS word at a byte address
typedef __attribute__((address_space(3))) unsigned char lds_u8;

__device__ __forceinline__ uint32_t pos_lo_x4(uint32_t p) {
    uint32_t r;
    asm volatile("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
                 : "=v"(r) : "v"(p));
    return r;
}
__device__ __forceinline__ uint32_t pos_hi_x4(uint32_t p) {
    uint32_t r;
    asm volatile("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1"
                 : "=v"(r) : "v"(p));
    return r;
}

}  // namespace
}  // namespace ldpc
