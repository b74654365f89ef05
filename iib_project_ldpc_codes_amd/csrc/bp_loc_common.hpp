// What the two local-edge kernels share: bp_loc_kernel (bp_loc.hpp) and bp_loc_chain_kernel
// (bp_loc_chain.hpp).  The check rule of a check pair, the row and table loads, the workgroup reductions
// and the compile-time switches.
#pragma once
#include "bp_device.hpp"

namespace ldpc {
namespace {

#ifndef LDPC_LOC_VGROUP
#define LDPC_LOC_VGROUP 1  // variable pairs per scheduling group (0: no barriers)
#endif
#ifndef LDPC_LOC_CGROUP
#define LDPC_LOC_CGROUP 1  // check pairs per scheduling group (0: no barriers)
#endif
#ifndef LDPC_LOC_EP_W0
#define LDPC_LOC_EP_W0 48  // early stop with posteriors: slab writes after syndromes with <= this many threads unsatisfied
#endif
#ifndef LDPC_LOC_PRIO
// wave priority by phase: the variable phase (LDS-bound gathers / scatters) at s_setprio 1, the
// check phase (VALU-bound) at 0 -- two co-resident workgroups in opposite phases then share the
// SIMD in favour of the one that feeds the LDS pipe.  Headline +1.9 % (28.94 -> 28.39 ms), early
// stop and Monte-Carlo +1-3 %; the reverse assignment -2.4 %, odd workgroups at 1 neutral.
#define LDPC_LOC_PRIO 1
#endif

// SGN (sum-product with early stop): every non-local v->c ratio carries its variable's hard
// decision in one bit; with the decisions of the pair's two local variables (lpar, from the
// thread's own decision bits: bit 0 the .x check's, bit 1 the .y check's parity of them) the
// pair's parities are the syndrome of the previous variable phase (returned: 1 = a check of
// the pair unsatisfied).  The bit is the ratio's mantissa LSB (a relative change of at most
// 2^-23, far below the rule's ~10-ulp error), so the check rule takes the inputs as they are:
// the parity is two v_bitop3 XOR chains and one OR per pair, no input needs its sign stripped,
// and the local edges (registers) carry no stamp.
// seed ^ the words of entries 2 .. N-1 (N <= D) of one half of x
template <int N, int D>
__device__ __forceinline__ uint32_t bits_parity(const float2 (&x)[D], bool hi, uint32_t seed) {
    auto w = [&](int j) { return __float_as_uint(hi ? x[j].y : x[j].x); };
    uint32_t p = seed;
    int j = 2;
#pragma unroll
    for (; j + 1 < N; j += 2) p = xor3u(p, w(j), w(j + 1));
    if (j < N) p ^= w(j);
    return p;
}
// One check pair: inputs 0 and 1 are the local edges l0, l1 (registers, overwritten with the outputs),
// the others the pair's row entries from word W of msg, in rows of Nc pairs.
// CL > 0 (the chained layout, bp_loc_chain_kernel): input slot 2 is the thread's chain register *chain,
// overwritten with that slot's output; the pair's rows hold the other D - 3 inputs.
// The pair is entry off + i of its class: a caller that knows part of the index at compile time passes it as off,
// and with W and Nc constants too every row access is one lane base (16 i or 8 i bytes) plus an immediate.
template <int D, int ALGO, bool MIXED = false, bool SGN = false, int CL = 0>
__device__ __forceinline__ int loc_check_pair(float *msg, int W, int Nc, int i, float2 &l0, float2 &l1, float alpha,
                                              uint32_t lpar = 0u, float2 *chain = nullptr, int off = 0) {
    constexpr int C = CL > 0 ? 1 : 0, U = D - 2 - C;
    float2 x[D];
    x[0] = l0;
    x[1] = l1;
    if constexpr (C) x[2] = *chain;
#pragma unroll
    for (int r = 0; r < U / 2; ++r) {
        const float4 f = *reinterpret_cast<const float4 *>(msg + W + r * 4 * Nc + 4 * off + 4 * i);
        x[2 + C + 2 * r] = make_float2(f.x, f.y);
        x[3 + C + 2 * r] = make_float2(f.z, f.w);
    }
    if constexpr (U % 2) x[D - 1] = *reinterpret_cast<const float2 *>(msg + W + (U / 2) * 4 * Nc + 2 * off + 2 * i);
    int unsat = 0;
    if constexpr (SGN) {  // raw parity words: the caller ORs them and tests bit 0 once
        // a mixed pair's .x check has D - 1 inputs: its pad slot holds the rule's output for the
        // padding input (an arbitrary LSB), not a variable's decision
        unsat = (int)(bits_parity<MIXED ? D - 1 : D, D>(x, false, lpar) | bits_parity<D, D>(x, true, lpar >> 1));
    }
    if constexpr (ALGO == 0) {
        if constexpr (MIXED) {  // the .x check has D - 1 edges: pad input R = 0
            x[D - 1].x = 0.0f;
            check_update_spa_pair_rwire<D, true>(x);
        } else {
            check_update_spa_pair_rwire<D>(x);
        }
    } else {
        float xa[D], xb[D];
#pragma unroll
        for (int j = 0; j < D; ++j) { xa[j] = x[j].x; xb[j] = x[j].y; }
        if constexpr (MIXED) {  // pad: an infinite magnitude changes no minimum or sign
            xa[D - 1] = __builtin_inff();
            check_update<1, D>(xa, alpha);
            check_update<1, D>(xb, alpha);
        } else if constexpr (D == 6) {
            check_update_ms6(xa, alpha);
            check_update_ms6(xb, alpha);
        } else {
            check_update<1, D>(xa, alpha);
            check_update<1, D>(xb, alpha);
        }
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = make_float2(xa[j], xb[j]);
    }
#pragma unroll
    for (int r = 0; r < U / 2; ++r)
        *reinterpret_cast<float4 *>(msg + W + r * 4 * Nc + 4 * off + 4 * i) =
            make_float4(x[2 + C + 2 * r].x, x[2 + C + 2 * r].y, x[3 + C + 2 * r].x, x[3 + C + 2 * r].y);
    if constexpr (U % 2) *reinterpret_cast<float2 *>(msg + W + (U / 2) * 4 * Nc + 2 * off + 2 * i) = x[D - 1];
    l0 = x[0];
    l1 = x[1];
    if constexpr (C) *chain = x[2];
    return unsat;
}

// a load whose index the compiler may not hoist out of the codeword loop (it would keep
// one 64-bit address per load live across the decode -- VGPRs the loop needs)
template <typename V>
__device__ __forceinline__ V ld_fresh(const V *p, int idx) {
    asm volatile("" : "+v"(idx));
    return p[idx];
}
// Row b of a [B][len] tensor as a raw buffer of `bytes` bytes: stride 0, no swizzle, and in the
// descriptor's last word only DATA_FORMAT (bits 18:15) = 4, a 32-bit element -- a zero there is the
// invalid format of an unbound resource; the untyped loads and stores below read no other field of
// it.  Base = the row start (a 64-bit scalar add: a batch past 4 GB stays clear of the 32-bit lane
// offsets).  The hardware's range check (offset >= bytes) returns 0 from a load past the row and
// drops a store past it, so no access below carries a guard of its own; every access is aligned to
// its own size and len % 4 = 0, so none straddles the row's end
// (tests/test_gpu_loc_row_io.py holds this with sentinels around every output row).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const void *row, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(row), 0, bytes, 0x00020000);
}
// Entry `entry` (a compile-time constant: the row's start) + lane of a thread-layout table of int32
// through the table's descriptor: the row's byte offset is the instruction's scalar offset, the
// lane's part one 32-bit byte offset (lane_bytes = 4 tid, made opaque where it is formed, so -- as
// with ld_fresh -- nothing per entry is held across the decode, and no 64-bit VALU address is formed)
__device__ __forceinline__ int32_t ld_row(__amdgpu_buffer_rsrc_t tab, int entry, uint32_t lane_bytes) {
    return (int32_t)__builtin_amdgcn_raw_buffer_load_b32(tab, lane_bytes, 4 * entry, 0);
}

// Workgroup-wide OR of a per-lane predicate with ONE barrier (__syncthreads_or reduces
// through a wave DPP chain, an LDS atomic and three barriers): each wave whose ballot is
// non-zero has lane 0 store 1 to flag[par]; after the barrier every thread reads it; thread 0
// then clears flag[par ^ 1] -- its previous readers are all past this barrier, and its next
// writers are behind the next one.  flag[] must be zero before the first call; alternate par.
__device__ __forceinline__ bool block_any(int pred, uint32_t *flag, int par) {
    if (__builtin_amdgcn_ballot_w64(pred != 0) != 0 && (threadIdx.x & (kWave - 1)) == 0) flag[par] = 1u;
    __syncthreads();
    const bool any = flag[par] != 0u;
    if (threadIdx.x == 0) flag[par ^ 1] = 0u;
    return any;
}
// block_any's count form: the number of waves' lanes with pred set (one LDS atomic per wave)
__device__ __forceinline__ uint32_t block_count(int pred, uint32_t *flag, int par) {
    const uint64_t bal = __builtin_amdgcn_ballot_w64(pred != 0);
    if (bal != 0 && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(&flag[par], (uint32_t)__popcll(bal));
    __syncthreads();
    const uint32_t c = flag[par];
    if (threadIdx.x == 0) flag[par ^ 1] = 0u;
    return c;
}

// 512 threads with up to 5 check pairs each: two workgroups per CU (4 waves per SIMD, <= 128
// VGPRs), so one workgroup's barrier waits overlap the other's work; else one workgroup
constexpr int loc_waves_per_simd(int T, int KP) { return T == 512 && KP <= 5 ? 4 : 1; }

}  // namespace
}  // namespace ldpc
