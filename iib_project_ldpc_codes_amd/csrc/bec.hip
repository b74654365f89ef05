// BEC erasure decoding: bec_kernel (one workgroup per codeword) and the bit-sliced kernels,
// with their launchers.
//
// Reference behaviour restated here:
//   message_passing.c:7-82         -> bec_kernel           (bit-exact)
#include <atomic>

#include "kernel_args.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {
namespace {

// ===========================================================================
// 1. BEC erasure decoding -- message_passing.c:7-82, bit-exact.
//
// One workgroup per codeword.  LDS: caller errors[] (int32), the ternary word
// (u8) and one byte per check.  The reference's per-slot check messages are
// never materialised: a slot addressed to an ERASED variable is known iff its
// check holds exactly one erasure, and then equals the parity of the check's
// known bits (message_passing.c:31-43); so each check publishes one byte
// cs = ne==1 ? parity : 2 and an erased variable takes the last cs != 2 over
// its checks in variable_to_check_list order (message_passing.c:55-62).
// vchk = -1 marks a (variable, check) pair where the check does not hold the
// variable exactly once: such a pair never assigns in the reference.
// ===========================================================================

template <int T, bool MC>
__global__ __launch_bounds__(T) void bec_kernel(BecArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int red[T / kWave];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int n = a.n, m = a.m, iters = a.max_iters;
    int32_t *errs = reinterpret_cast<int32_t *>(smem);
    uint8_t *mvc = smem + ((iters * 4 + 15) & ~15);
    uint8_t *cs = mvc + ((n + 15) & ~15);
    const int32_t *cvar = a.cvar + (size_t)b * a.graph_stride;
    const int32_t *vchk = a.vchk + (size_t)b * a.graph_stride;

    int init_cnt = 0;
    if (MC) {
        const uint64_t cw = a.first_cw + b;
        for (int g4 = tid; g4 < (n + 3) >> 2; g4 += T) {  // one Philox block per four variables
            const uint4 r = chan_block(a.ch, cw, g4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (4 * g4 + q >= n) break;
                const uint8_t x = u01(pick4(r, q)) < a.ch.p ? 2 : 0;  // chan_bec
                mvc[4 * g4 + q] = x;
                init_cnt += (x == 2);
            }
        }
        for (int i = tid; i < iters; i += T) errs[i] = 0;
    } else {
        const uint8_t *w = a.words + b * n;
        for (int v = tid; v < n; v += T) mvc[v] = w[v];
        const int32_t *e = a.errors + b * iters;
        for (int i = tid; i < iters; i += T) errs[i] = e[i];
    }
    __syncthreads();
    const int initial = MC ? block_sum<T>(init_cnt, red) : 0;

    int prev1 = 0, prev2 = 0;  // errors[it-1], errors[it-2] after accumulation
    int it;
    for (it = 0; it < iters; ++it) {
        if (it >= 2 && prev1 == prev2) {  // message_passing.c:16-19 (absorbing)
            for (int i = it + tid; i < iters; i += T) errs[i] = prev1;
            it = iters;
            break;
        }
        // check phase (reads the previous word only)
        for (int c = tid; c < m; c += T) {
            const int s0 = a.dc > 0 ? c * a.dc : a.cptr[c];
            const int s1 = a.dc > 0 ? s0 + a.dc : a.cptr[c + 1];
            int ne = 0, par = 0;
            for (int s = s0; s < s1; ++s) {
                const int x = mvc[cvar[s]];
                ne += (x == 2);
                par ^= (x & 1);
            }
            cs[c] = (uint8_t)(ne == 1 ? par : 2);
        }
        __syncthreads();
        // variable phase: erased variables take the last known check message
        int cnt = 0;
        for (int v = tid; v < n; v += T) {
            int x = mvc[v];
            if (x == 2) {
                const int e0 = a.dv > 0 ? v * a.dv : a.vptr[v];
                const int e1 = a.dv > 0 ? e0 + a.dv : a.vptr[v + 1];
                for (int e = e0; e < e1; ++e) {
                    const int c = vchk[e];
                    if (c >= 0) {
                        const int y = cs[c];
                        if (y != 2) x = y;
                    }
                }
                mvc[v] = (uint8_t)x;
                cnt += (x == 2);
            }
        }
        const int base = errs[it];  // read before block_sum's barriers, written after
        const int total = block_sum<T>(cnt, red);
        const int cur = base + total;
        if (tid == 0) errs[it] = cur;
        prev2 = prev1;
        prev1 = cur;
        if (total == 0) break;  // message_passing.c:76-78
    }
    __syncthreads();
    if (MC) {
        int32_t *tr = a.trial + b * (size_t)(iters + 1);
        for (int i = tid; i <= iters; i += T) tr[i] = i == 0 ? initial : errs[i - 1];
        if (tid == 0) a.its[b] = it;
    } else {
        uint8_t *w = a.words + b * n;
        for (int v = tid; v < n; v += T) w[v] = mvc[v];
        int32_t *e = a.errors + b * iters;
        for (int i = tid; i < iters; i += T) e[i] = errs[i];
        if (tid == 0) a.its[b] = it;
    }
}

// ---------------------------------------------------------------------------
// 1b. BEC Monte-Carlo, bit-sliced: the same decoder (message_passing.c:7-82 with
// the all-zero codeword of parallel_simulator.py:222) for 32*W codewords per
// workgroup at once.  Bit b of word w of variable v is "codeword 32w+b has v
// erased".  With the all-zero codeword every known bit is 0, so the parity of a
// check's known bits is 0 and only the erasure planes evolve:
//   check c:    One[c] = codewords where exactly one of c's slots is erased
//               (carry-save: two |= one & e; one |= e; One = one & ~two)
//   variable v: E[v] &= ~OR_{edges e of v, vchk[e] >= 0} One[vchk[e]]
// which is bec_kernel's rule (an erased variable takes any known check message;
// known messages are 0) bit for bit, Jacobi (One is built from the old planes).
// Running every codeword for all iterations in lockstep is exact: a stalled or
// finished codeword is a fixed point, so its counts repeat (message_passing.c:
// 16-19 fills errors[it] = errors[it-1]; after the break at a zero count the
// caller's zeros remain).  Per-codeword counts per iteration come from one LDS
// atomic per resolved (codeword, variable); its = the first iteration whose
// count is zero, else iters; the decode stops once no codeword changes.
// Channel: bit = chan_bec(cw, v) (the stream of bec_kernel / oracle_channel),
// 32 codewords per half-wave, one Philox block per lane per 4 variables,
// transposed into the planes by ballots.  Output: trial[b][iters+1] and its[b]
// in bec_kernel's MC layout, so mc_cutoff / mc_reduce apply unchanged.
// LDS: E[n][W], One[m][W] (u32), cnt[32W], its[32W], 3 change flags.
// ---------------------------------------------------------------------------
// Plane words: P = uint32_t (32 codewords, W words per variable) or uint8_t (8
// codewords, W = 1: planes of n + m bytes, for graphs whose u32 planes do not fit).
template <typename P, int W> struct BitsVec;
template <> struct BitsVec<uint32_t, 1> { typedef uint32_t T; };
template <> struct BitsVec<uint32_t, 2> { typedef uint2 T; };
template <> struct BitsVec<uint32_t, 4> { typedef uint4 T; };
template <> struct BitsVec<uint8_t, 1> { typedef uint8_t T; };

template <typename P, int W>
__device__ __forceinline__ void bits_load(const P *p, uint32_t (&x)[W]) {
    const typename BitsVec<P, W>::T v = *reinterpret_cast<const typename BitsVec<P, W>::T *>(p);
    if constexpr (W == 1) x[0] = v;
    if constexpr (W == 2) { x[0] = v.x; x[1] = v.y; }
    if constexpr (W == 4) { x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
}
template <typename P, int W>
__device__ __forceinline__ void bits_store(P *p, const uint32_t (&x)[W]) {
    typename BitsVec<P, W>::T v;
    if constexpr (W == 1) v = (P)x[0];
    if constexpr (W == 2) v = make_uint2(x[0], x[1]);
    if constexpr (W == 4) v = make_uint4(x[0], x[1], x[2], x[3]);
    *reinterpret_cast<typename BitsVec<P, W>::T *>(p) = v;
}

template <int T, int W, typename P>
__global__ __launch_bounds__(T) void bec_mc_bits_kernel(BecArgs a, int B) {
    static_assert(T % 64 == 0, "lane groups of BITS codewords tile the waves");
    constexpr int BITS = 8 * sizeof(P);  // codewords per plane word
    constexpr int NB = BITS * W;         // codewords per workgroup
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int n = a.n, m = a.m, iters = a.max_iters;
    P *Ev = reinterpret_cast<P *>(smem);  // [n][W]
    P *On = Ev + (size_t)n * W;           // [m][W]
    int *cnt = reinterpret_cast<int *>(smem + ((((size_t)n + m) * W * sizeof(P) + 15) & ~(size_t)15));  // [NB]
    int *itsl = cnt + NB;                                                       // [NB]
    uint32_t *flag = reinterpret_cast<uint32_t *>(itsl + NB);                   // [3] "some codeword changed"
    const int64_t b0 = (int64_t)blockIdx.x * NB;
    const int nloc = (int)min((int64_t)NB, (int64_t)B - b0);  // codewords of this block with trial rows

    for (int i = tid; i < NB; i += T) {
        cnt[i] = 0;
        itsl[i] = iters;
    }
    if (tid < 3) flag[tid] = 0;
    __syncthreads();
    // ---- channel: a group of BITS lanes = one (group g of 4 variables, word w); lane = codeword bit ----
    {
        const int ngr = (n + 3) >> 2;
        const int bit = tid & (BITS - 1);
        const int shift = (tid & (kWave - 1)) & ~(BITS - 1);  // this group's bits in the wave ballot
        int local[W];
#pragma unroll
        for (int w = 0; w < W; ++w) local[w] = 0;
        for (int base = tid / BITS; base < ngr * W; base += T / BITS) {
            const int g = base / W, w = base - g * W;
            const uint64_t cw = a.first_cw + (uint64_t)(b0 + BITS * w + bit);
            const uint4 r = philox_block((uint32_t)g, 0u, (uint32_t)cw, (uint32_t)(cw >> 32), a.ch.k0, a.ch.k1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = 4 * g + j;
                const bool er = v < n && u01(pick4(r, j)) < a.ch.p;
                const uint64_t bal = __ballot(er);
                local[w] += er;
                if (bit == 0 && v < n) Ev[(size_t)v * W + w] = (P)(bal >> shift);
            }
        }
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (local[w]) atomicAdd(&cnt[BITS * w + bit], local[w]);
    }
    __syncthreads();
    for (int i = tid; i < nloc; i += T) a.trial[(size_t)(b0 + i) * (iters + 1)] = cnt[i];

    int it = 0;
    for (; it < iters; ++it) {
        // ---- check phase (reads the previous planes only) ----
        for (int c = tid; c < m; c += T) {
            const int s0 = a.dc > 0 ? c * a.dc : a.cptr[c];
            const int s1 = a.dc > 0 ? s0 + a.dc : a.cptr[c + 1];
            uint32_t one[W], two[W];
#pragma unroll
            for (int w = 0; w < W; ++w) one[w] = two[w] = 0u;
            for (int s = s0; s < s1; ++s) {
                uint32_t e[W];
                bits_load<P, W>(Ev + (size_t)a.cvar[s] * W, e);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    two[w] |= one[w] & e[w];
                    one[w] |= e[w];
                }
            }
#pragma unroll
            for (int w = 0; w < W; ++w) one[w] &= ~two[w];
            bits_store<P, W>(On + (size_t)c * W, one);
        }
        __syncthreads();
        if (tid == 0) flag[(it + 1) % 3] = 0u;  // next iteration's flag (last read before this barrier)
        // ---- variable phase ----
        uint32_t changed = 0u;
        for (int v = tid; v < n; v += T) {
            uint32_t e[W], any = 0u;
            bits_load<P, W>(Ev + (size_t)v * W, e);
#pragma unroll
            for (int w = 0; w < W; ++w) any |= e[w];
            if (!any) continue;
            const int e0 = a.dv > 0 ? v * a.dv : a.vptr[v];
            const int e1 = a.dv > 0 ? e0 + a.dv : a.vptr[v + 1];
            uint32_t r[W];
#pragma unroll
            for (int w = 0; w < W; ++w) r[w] = 0u;
            for (int x = e0; x < e1; ++x) {
                const int c = a.vchk[x];
                if (c < 0) continue;
                uint32_t o[W];
                bits_load<P, W>(On + (size_t)c * W, o);
#pragma unroll
                for (int w = 0; w < W; ++w) r[w] |= o[w];
            }
            uint32_t ne[W];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                r[w] &= e[w];  // resolved this iteration
                ne[w] = e[w] & ~r[w];
                changed |= r[w];
            }
            bits_store<P, W>(Ev + (size_t)v * W, ne);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                uint32_t q = r[w];
                while (q) {
                    const int b = __builtin_ctz(q);
                    q &= q - 1u;
                    atomicSub(&cnt[BITS * w + b], 1);
                }
            }
        }
        if (__ballot(changed != 0u) && (tid & (kWave - 1)) == 0) atomicOr(&flag[it % 3], 1u);
        __syncthreads();
        for (int i = tid; i < NB; i += T) {
            const int c = cnt[i];
            if (c == 0 && itsl[i] == iters) itsl[i] = it;
            if (i < nloc) a.trial[(size_t)(b0 + i) * (iters + 1) + it + 1] = c;
        }
        if (!flag[it % 3]) {  // nothing changed: every codeword is at its fixed point
            for (int i = tid; i < nloc; i += T) {
                int32_t *tr = a.trial + (size_t)(b0 + i) * (iters + 1);
                const int c = cnt[i];
                for (int j = it + 2; j <= iters; ++j) tr[j] = c;
            }
            break;
        }
    }
    __syncthreads();
    for (int i = tid; i < nloc; i += T) a.its[b0 + i] = itsl[i];
}

// ---------------------------------------------------------------------------
// 1c. BEC batch decode, bit-sliced: bec_kernel's non-MC contract (arbitrary
// words, caller errors[] accumulated and steering the stall test of
// message_passing.c:16-19) for H = 4*sizeof(P) codewords per plane word.
// A variable's word holds "erased" bits (low H) and value bits (high H, the
// byte's bit 0 when not erased, 0 when erased); a check's word holds "exactly
// one slot erased" bits (low) and the parity of its known bits (high), i.e.
// bec_kernel's cs = ne==1 ? parity : 2.  Variable phase, in
// variable_to_check_list order: sel = One[c] & erased & active,
// val = (val & ~sel) | (parity & sel) -- the last known check message wins
// (message_passing.c:55-62) -- and the variable is resolved iff some sel was set.
// Codeword control (counts, stall test, zero-count break) is per codeword in
// registers of lane i < NB; codewords that have stopped are masked out of the
// variable phase ("active"), so a stalled word is frozen exactly as the
// reference's early return leaves it.  When no codeword changed in an
// iteration every active codeword is at a fixed point and its remaining
// iterations (count fixed, caller errors[] still added and tested) are
// replayed by its lane without touching the graph.
// Output rewrites only the bytes that were 2 on input (a known byte is never
// changed by the reference, whatever its value).
// LDS: X[n][W], C[m][W] plane words, cnt[NB], act[W], 2 change flags, done.
// ---------------------------------------------------------------------------
template <int T, int W, typename P>
__global__ __launch_bounds__(T) void bec_dec_bits_kernel(BecArgs a, int B) {
    constexpr int H = 4 * (int)sizeof(P);  // codewords per plane word
    constexpr uint32_t LO = (1u << H) - 1u;
    constexpr int NB = H * W;  // codewords per workgroup (<= 64: control lanes in wave 0)
    static_assert(NB <= kWave, "control lanes must sit in wave 0");
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int n = a.n, m = a.m, iters = a.max_iters;
    P *Xv = reinterpret_cast<P *>(smem);  // [n][W]
    P *Xc = Xv + (size_t)n * W;           // [m][W]
    int *cnt = reinterpret_cast<int *>(smem + ((((size_t)n + m) * W * sizeof(P) + 15) & ~(size_t)15));  // [NB]
    uint32_t *act = reinterpret_cast<uint32_t *>(cnt + NB);  // [W]
    uint32_t *flag = act + W;                                 // [2] changed, [2] all stopped
    const int64_t b0 = (int64_t)blockIdx.x * NB;
    const int nloc = (int)min((int64_t)NB, (int64_t)B - b0);

    for (int i = tid; i < NB; i += T) cnt[i] = 0;
    if (tid < 3) flag[tid] = 0u;
    if (tid < W) act[tid] = (1u << min(max(nloc - tid * H, 0), H)) - 1u;  // codewords with rows
    __syncthreads();
    // ---- words -> planes: thread (w, v) gathers byte v of the word's H rows (lanes = consecutive v) ----
#pragma unroll
    for (int w = 0; w < W; ++w) {
        int lc[H];
#pragma unroll
        for (int j = 0; j < H; ++j) lc[j] = 0;
        for (int v = tid; v < n; v += T) {
            uint32_t x = 0u;
#pragma unroll
            for (int j = 0; j < H; ++j) {
                const int i = w * H + j;
                const uint32_t y = i < nloc ? a.words[(size_t)(b0 + i) * n + v] : 0u;
                const bool er = y == 2u;
                x |= (uint32_t)er << j | (er ? 0u : (y & 1u)) << (H + j);
                lc[j] += er;
            }
            Xv[(size_t)v * W + w] = (P)x;
        }
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const int s = wave_sum(lc[j]);
            if (lane == 0 && s) atomicAdd(&cnt[w * H + j], s);
        }
    }
    // control state of codeword tid (tid < nloc)
    int p1 = 0, p2 = 0, its = iters;
    bool done = tid >= nloc;
    int32_t *er = a.errors + (size_t)(b0 + min(tid, max(nloc - 1, 0))) * iters;
    __syncthreads();

    for (int it = 0; it < iters; ++it) {
        // ---- check phase (reads the previous planes only) ----
        for (int c = tid; c < m; c += T) {
            const int s0 = a.dc > 0 ? c * a.dc : a.cptr[c];
            const int s1 = a.dc > 0 ? s0 + a.dc : a.cptr[c + 1];
            uint32_t one[W], two[W], par[W];
#pragma unroll
            for (int w = 0; w < W; ++w) one[w] = two[w] = par[w] = 0u;
            for (int s = s0; s < s1; ++s) {
                uint32_t x[W];
                bits_load<P, W>(Xv + (size_t)a.cvar[s] * W, x);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const uint32_t e = x[w] & LO;
                    two[w] |= one[w] & e;
                    one[w] |= e;
                    par[w] ^= x[w] >> H;
                }
            }
#pragma unroll
            for (int w = 0; w < W; ++w) one[w] = (one[w] & ~two[w]) | (par[w] & LO) << H;
            bits_store<P, W>(Xc + (size_t)c * W, one);
        }
        __syncthreads();
        // ---- variable phase: active erased variables take the last known check message ----
        uint32_t av[W];
#pragma unroll
        for (int w = 0; w < W; ++w) av[w] = act[w];
        uint32_t changed = 0u;
        for (int v = tid; v < n; v += T) {
            uint32_t x[W], any = 0u;
            bits_load<P, W>(Xv + (size_t)v * W, x);
#pragma unroll
            for (int w = 0; w < W; ++w) any |= x[w] & av[w];
            if (!any) continue;
            const int e0 = a.dv > 0 ? v * a.dv : a.vptr[v];
            const int e1 = a.dv > 0 ? e0 + a.dv : a.vptr[v + 1];
            uint32_t val[W], res[W];
#pragma unroll
            for (int w = 0; w < W; ++w) val[w] = res[w] = 0u;
            for (int e = e0; e < e1; ++e) {
                const int c = a.vchk[e];
                if (c < 0) continue;
                uint32_t y[W];
                bits_load<P, W>(Xc + (size_t)c * W, y);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const uint32_t sel = y[w] & x[w] & av[w];  // low bits only (av)
                    val[w] = (val[w] & ~sel) | ((y[w] >> H) & sel);
                    res[w] |= sel;
                }
            }
#pragma unroll
            for (int w = 0; w < W; ++w) {
                x[w] = (x[w] & ~res[w]) | val[w] << H;
                changed |= res[w];
            }
            bits_store<P, W>(Xv + (size_t)v * W, x);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                uint32_t q = res[w];
                while (q) {
                    const int b = __builtin_ctz(q);
                    q &= q - 1u;
                    atomicSub(&cnt[w * H + b], 1);
                }
            }
        }
        if (__ballot(changed != 0u) && lane == 0) atomicOr(&flag[it & 1], 1u);
        __syncthreads();
        // ---- control: message_passing.c:70-78 per codeword, then the stall test of the next iteration ----
        if (tid < kWave) {
            if (!done) {
                const bool chg = flag[it & 1] != 0u;
                const int c = cnt[tid];
                int cur = er[it] + c;
                er[it] = cur;
                p2 = p1;
                p1 = cur;
                if (c == 0) {
                    done = true;
                    its = it;
                } else {
                    for (int t = it + 1; t < iters; ++t) {
                        if (t >= 2 && p1 == p2) {  // message_passing.c:16-19
                            for (int j = t; j < iters; ++j) er[j] = p1;
                            done = true;
                            break;
                        }
                        if (chg) break;
                        cur = er[t] + c;  // fixed point: replay iteration t
                        er[t] = cur;
                        p2 = p1;
                        p1 = cur;
                    }
                    if (!chg) done = true;  // its stays iters
                }
            }
            const uint64_t alive = __ballot(!done);
            if (tid == 0) {
#pragma unroll
                for (int w = 0; w < W; ++w) act[w] = (uint32_t)(alive >> (w * H)) & LO;
                flag[(it + 1) & 1] = 0u;
                flag[2] = alive == 0ull;
            }
        }
        __syncthreads();
        if (flag[2]) break;
    }
    if (tid < nloc) a.its[b0 + tid] = its;
    // ---- planes -> words: rewrite the bytes that were erased on input ----
#pragma unroll
    for (int w = 0; w < W; ++w) {
        for (int v = tid; v < n; v += T) {
            const uint32_t x = Xv[(size_t)v * W + w];
#pragma unroll
            for (int j = 0; j < H; ++j) {
                const int i = w * H + j;
                if (i < nloc) {
                    uint8_t *p = a.words + (size_t)(b0 + i) * n + v;
                    if (*p == 2u) *p = ((x >> j) & 1u) ? 2u : (uint8_t)((x >> (H + j)) & 1u);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// 2. Launchers.  bec_plan (bec_plan.cpp) names the kernel, its shape, grid and LDS; the code
// below fills the arguments and launches that instantiation.
// ---------------------------------------------------------------------------
template <bool DEC, int T, int W, typename P>
hipError_t launch_bits_as(const BecPlan &p, const BecArgs &a, int B, hipStream_t stream) {
    const dim3 grid((unsigned)p.grid), block(T);
    if constexpr (DEC) return launch_lds(bec_dec_bits_kernel<T, W, P>, grid, block, p.lds, stream, a, B);
    else return launch_lds(bec_mc_bits_kernel<T, W, P>, grid, block, p.lds, stream, a, B);
}

// The bit-sliced instantiations: the rows of the shape table (kernel_shapes.hpp), from which
// bec_plan takes the shape it names.  The kernels lie in the code object in the order of the rows
// (and Decode's before Monte-Carlo's): it is kept as it was measured.
template <bool DEC>
hipError_t launch_bits(const BecPlan &p, const BecArgs &a, int B, hipStream_t stream) {
#define LDPC_ROW(T, WW, P, TAG) \
    if (p.threads == T && p.W == WW && p.plane == (int)sizeof(P)) return launch_bits_as<DEC, T, WW, P>(p, a, B, stream);
    LDPC_BEC_BITS_SHAPES(LDPC_ROW)
#undef LDPC_ROW
    return hipErrorInvalidValue;  // a shape without a row: the plan gives none
}

template <bool MC>
hipError_t launch_word(const BecPlan &p, const BecArgs &a, hipStream_t stream) {
#define LDPC_ROW(T) \
    if (p.threads == T) return launch_lds(bec_kernel<T, MC>, dim3((unsigned)p.grid), dim3(T), p.lds, stream, a);
    LDPC_BEC_WORD_SHAPES(LDPC_ROW)
#undef LDPC_ROW
    return hipErrorInvalidValue;
}

// MC: the fused-channel forms (bec_kernel<T, true>, bec_mc_bits_kernel).  hipErrorInvalidValue: no
// kernel holds the graph (said before an empty batch is let through, as ever).
template <bool MC>
hipError_t launch_bec(const BecPlan &p, const BecArgs &a, int B, hipStream_t stream) {
    switch (p.kernel) {
        case MC ? BecKernel::McBits : BecKernel::DecBits: return launch_bits<!MC>(p, a, B, stream);
        case BecKernel::Word: return B <= 0 ? hipSuccess : launch_word<MC>(p, a, stream);
        default: return hipErrorInvalidValue;
    }
}

BecArgs bec_args(int n, int m, int dv, int dc, int max_iters) {
    BecArgs a{};
    a.n = n;
    a.m = m;
    a.dv = dv;
    a.dc = dc;
    a.max_iters = max_iters;
    return a;
}

BecArgs bec_args(const ldpc_graph &g, int max_iters) {
    BecArgs a = bec_args(g.n, g.m, g.dv, g.dc, max_iters);
    a.cvar = g.cvar;
    a.cptr = g.cptr;
    a.vptr = g.vptr;
    a.vchk = g.vchk;
    return a;
}

void mc_args(BecArgs &a, float p, float p2, uint64_t seed, uint64_t first_cw, int32_t *trial, int32_t *trial_its) {
    a.ch = make_chan(0, p, p2, seed);
    a.first_cw = first_cw;
    a.trial = trial;
    a.its = trial_its;
}

// Test-only bound on the peeling decoder's frontier capacity (ldpc_debug_peel_cap); 0: none.
std::atomic<int> g_peel_cap{0};

}  // namespace

hipError_t launch_bec_decode(const ldpc_graph &g, uint8_t *d_words, int B, int max_iters,
                             int32_t *d_errors, int32_t *d_its, hipStream_t stream) {
    BecArgs a = bec_args(g, max_iters);
    a.words = d_words;
    a.errors = d_errors;
    a.its = d_its;
    return launch_bec<false>(bec_plan(g.n, g.m, g.dc, B, max_iters, BecMode::Decode, 0), a, B, stream);
}

hipError_t launch_mc_bec(const ldpc_graph &g, float p, float p2, uint64_t seed, uint64_t first_cw, int B,
                         int max_iters, int32_t *trial, int32_t *trial_its, hipStream_t stream) {
    BecArgs a = bec_args(g, max_iters);
    mc_args(a, p, p2, seed, first_cw, trial, trial_its);
    return launch_bec<true>(bec_plan(g.n, g.m, g.dc, B, max_iters, BecMode::Mc, 0), a, B, stream);
}

hipError_t launch_mc_bec_ensemble(int n, int dv, int dc, const int32_t *check_lookup, const int32_t *variable_lookup,
                                  float p, uint64_t seed, uint64_t first_cw, int B, int max_iters, int32_t *trial,
                                  int32_t *trial_its, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    const int m = n * dv / dc;
    const BecPlan plan = bec_plan(n, m, dc, B, max_iters, BecMode::EnsMc, g_peel_cap.load());
    if (plan.kernel == BecKernel::Peel)
        return launch_mc_bec_peel(plan, n, m, dv, dc, check_lookup, variable_lookup, p, seed, first_cw, max_iters,
                                  trial, trial_its, stream);
    BecArgs a = bec_args(n, m, dv, dc, max_iters);
    a.cvar = check_lookup;
    a.vchk = variable_lookup;
    a.graph_stride = (int64_t)n * dv;
    mc_args(a, p, 0.0f, seed, first_cw, trial, trial_its);
    return launch_bec<true>(plan, a, B, stream);
}

void peel_cap(int F) { g_peel_cap = F > 0 ? F : 0; }

}  // namespace ldpc
