// bp_lds_kernel: the LDS-resident (3,6) soft decoder, and its launch ladder.
#include "bp_device.hpp"

namespace ldpc {
namespace {

#ifndef LDPC_VAR_PAIRS
#define LDPC_VAR_PAIRS 1  // variable pairs per sched_barrier group in the LDS kernel's variable phase
#endif
#ifndef LDPC_CHECK_PAIRS_UNROLL
#define LDPC_CHECK_PAIRS_UNROLL 2  // check pairs per iteration of the LDS kernel's check loop (1: 1.4 % slower)
#endif
// ---------------------------------------------------------------------------
// 2a. Regular fast path: whole codeword resident in LDS.
//   LDS  msg[S + dummies] fp32, S = lds_pair_span(m, DC): check pairs (2q, 2q+1)
//        interleaved edge by edge ([q][edge][2], lds_pair_pos), hs[...] u8 hard
//        decision per position (ET only), curve (MC only).
//   Thread t owns check pairs t, t+T, ... and the variables of lane positions
//   p = t + i*T (i < VPT) of the host-built conflict-aware layout: every 32
//   consecutive positions (one half-wave LDS access) hit 32 distinct banks as far
//   as the graph allows; padding positions address private dummy positions.
//   Positions (packed 2 x 16 bit) and channel LLRs stay in VGPRs for the whole
//   decode.  Iteration = check phase (one conflict-free ds_read_b64 /
//   ds_write_b64 per edge of a pair; the update runs on float2, both checks in
//   every packed op) | barrier | variable phase (variables in pairs on float2:
//   DV gathers, posterior, extrinsic write-back) | barrier.  Channel LLRs in and
//   posteriors out are staged through LDS so their HBM traffic stays coalesced.
// ---------------------------------------------------------------------------
template <int DV, int DC, int T, int VPT, int ALGO, bool ET, bool MC>
__global__ __launch_bounds__(T) void bp_lds_kernel(BpArgs a) {
    static_assert(DC % 2 == 0, "pair layout: the ET parity reads whole words");
    static_assert(!ET || VPT <= 32, "early stop keeps one decision bit per lane in a 32-bit mask");
    extern __shared__ __align__(16) unsigned char smem[];
    float *msg = reinterpret_cast<float *>(smem);
    const int Ep = a.E + kLdsDummy;  // a.E = lds_pair_span(m, DC)
    uint8_t *hs = smem + (size_t)Ep * 4;
    int *curve = reinterpret_cast<int *>(smem + (((size_t)Ep * 5 + 15) & ~(size_t)15));
    const int tid = threadIdx.x;
    const int n = a.n, m = a.m, E = a.E, iters = a.max_iters;
    const int npairs = (m + 1) >> 1;
    constexpr int NS = VPT * DV;  // positions reached through my variables
    // The packed positions carry the dynamic LDS base (in words; not 0 when the
    // kernel also holds static LDS -- __syncthreads_or reduces through LDS), so
    // one SDWA shift yields the absolute address of a message.
    const int lpos0 = (int)((uint32_t)(size_t)(lds_u8 *)smem >> 2);
    uint8_t *hsb = hs - lpos0;  // hsb[address >> 2] = hs[position]

    // packed positions: codeword-independent, built once per workgroup
    uint32_t sp[(NS + 1) / 2];
#pragma unroll
    for (int q = 0; q < (NS + 1) / 2; ++q) sp[q] = 0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
#pragma unroll
        for (int j = 0; j < DV; ++j) {
            const int q = i * DV + j;
            sp[q >> 1] |= (uint32_t)(a.lane_slot[(tid + i * T) * DV + j] + lpos0) << (16 * (q & 1));
        }
    }
    // PF: the next codeword's channel LLRs are loaded into registers (v = tid + k*T,
    // n <= VPT*T) while the current one writes its outputs, so a persistent
    // workgroup never waits for HBM between codewords
    constexpr bool PF = LDPC_LDS36_PREFETCH && !MC && !ET;  // (early stop: 2.6 % slower, not used)
    float nx[PF ? VPT : 1];
    if constexpr (PF) {
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const int v = tid + k * T;
            nx[k] = v < n && (int)blockIdx.x < a.B ? a.llr[(size_t)blockIdx.x * n + v] : 0.0f;
        }
    }

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        // ---- stage the channel LLRs (coalesced) ----
        __syncthreads();  // previous codeword fully drained (msg, curve)
        if (MC) {
            for (int i = tid; i <= iters; i += T) curve[i] = 0;
        }
        int err0 = 0;
        if constexpr (PF) {
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                const int v = tid + k * T;
                if (v < n) msg[v] = to_msg<ALGO>(nx[k]);
            }
        } else {
            for (int v = tid; v < n; v += T) {
                const float l = MC ? chan_soft(a.ch, cw, v) : a.llr[(size_t)b * n + v];
                msg[v] = to_msg<ALGO>(l);
                err0 += (l < 0.0f);
            }
        }
        int lv[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) lv[i] = a.lane_var[tid + i * T];
        __syncthreads();
        float L[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) L[i] = lv[i] >= 0 ? msg[lv[i]] : 0.0f;
        // absolute LDS byte address of my variable i's edge j, and the word there
        auto addr = [&](int i, int j) -> uint32_t {
            const int q = i * DV + j;
            return (q & 1) ? pos_hi_x4(sp[q >> 1]) : pos_lo_x4(sp[q >> 1]);
        };
        auto at = [](uint32_t ba) -> lds_f32 & { return *(lds_f32 *)(size_t)ba; };
        __syncthreads();  // staging read before the message initialisation overwrites it
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const float w = v2c_rwire<ALGO>(L[i]);
#pragma unroll
            for (int j = 0; j < DV; ++j) at(addr(i, j)) = w;
        }
        __syncthreads();
        if (MC) {
            const int w = wave_sum(err0);
            if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[0], w);
        }

        // variable phase; FINAL (the last fixed-count iteration) keeps the
        // posteriors in registers instead of writing extrinsic messages.
        float pr[MC ? 1 : VPT];
        if constexpr (!MC) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) pr[i] = L[i];
        }
        // PROD (sum-product, no early stop): L holds E = 2^channel from here on, the
        // check phase leaves ratios r = 2^c2v in LDS, and the variable phase forms
        // each edge's extrinsic ratio E * prod_{k != j} r_k by prefix / suffix
        // products -- no v_log_f32 per edge in the check phase, a v_rcp_f32 in place
        // of the v_exp_f32 here.  The posterior (FINAL) is L + sum log2 r_j in the
        // log-domain order, L = log2(E); MC tests post < 1.
        constexpr bool PROD = ALGO == 0;
        if constexpr (PROD) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) L[i] = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(L[i], -126.0f, 126.0f));
        }
        // ET: a variable's hard-decision bytes are rewritten only when its decision
        // changes (bit i of hb = the decision last written for lane i; hfirst makes
        // the first variable phase of a codeword write them all)
        uint32_t hb = 0u;
        bool hfirst = true;
        auto put_hard = [&](int i, bool h, const uint32_t(&ad)[DV]) {
            if (hfirst || ((hb >> i) & 1u) != (uint32_t)h) {
#pragma unroll
                for (int j = 0; j < DV; ++j) hsb[ad[j] >> 2] = (uint8_t)h;
            }
            hb = (hb & ~(1u << i)) | ((uint32_t)h << i);
        };
        auto llr_log2 = [&](int i) -> float {  // PROD: channel LLR of lane i, message units
            // log2(E) restores it to ~1e-7 absolute; a value clamped at staging
            // (|LLR| > 87 nats) is re-read from the input instead
            float l = __builtin_amdgcn_logf(L[i]);
            if (__builtin_expect(fabsf(l) >= 126.0f, 0)) {
                const int vv = a.lane_var[tid + i * T];
                l = vv >= 0 && !MC ? to_msg<ALGO>(a.llr[(size_t)b * n + vv]) : 0.0f;
            }
            return l;
        };
        auto var_phase_prod = [&](auto final_tag) {
            constexpr bool FINAL = decltype(final_tag)::value;
            int errs = 0;
            auto edges = [&](auto &cv, auto Ev, auto put_j) {
                // cv[j]: ratios of this variable's edges; put_j(j, wire)
                decltype(Ev) pre[DV];
                pre[0] = Ev;
#pragma unroll
                for (int j = 1; j < DV; ++j) pre[j] = pre[j - 1] * cv[j - 1];
                auto suf = cv[DV - 1];
                put_j(DV - 1, pre[DV - 1]);
#pragma unroll
                for (int j = DV - 2; j >= 0; --j) {
                    put_j(j, pre[j] * suf);
                    if (j > 0) suf = suf * cv[j];
                }
                return pre[DV - 1] * cv[DV - 1];  // posterior ratio
            };
#pragma unroll
            for (int i = 0; i + 1 < VPT; i += 2) {
                uint32_t a0[DV], a1[DV];
                float2 cv[DV];
#pragma unroll
                for (int j = 0; j < DV; ++j) {
                    a0[j] = addr(i, j);
                    a1[j] = addr(i + 1, j);
                }
#pragma unroll
                for (int j = 0; j < DV; ++j) cv[j] = make_float2(at(a0[j]), at(a1[j]));
                if constexpr (FINAL) {
                    float2 s = make_float2(llr_log2(i), llr_log2(i + 1));
#pragma unroll
                    for (int j = 0; j < DV; ++j)
                        s = s + make_float2(__builtin_amdgcn_logf(cv[j].x), __builtin_amdgcn_logf(cv[j].y));
                    if constexpr (!MC) { pr[i] = s.x; pr[i + 1] = s.y; }
                } else {
                    const float2 post = edges(cv, make_float2(L[i], L[i + 1]), [&](int j, float2 R) {
                        const float2 w = ratio_wire2(R);
                        at(a0[j]) = w.x;
                        at(a1[j]) = w.y;
                    });
                    if constexpr (ET) {
                        put_hard(i, post.x < 1.0f, a0);
                        put_hard(i + 1, post.y < 1.0f, a1);
                        if constexpr (!MC) {  // prod r_j (no E: cannot overflow); logged at the end
                            float2 pq = cv[0];
#pragma unroll
                            for (int j = 1; j < DV; ++j) pq = pq * cv[j];
                            pr[i] = pq.x;
                            pr[i + 1] = pq.y;
                        }
                    }
                    if constexpr (MC)
                        errs += ((a0[0] < 4u * (E + lpos0)) & (post.x < 1.0f)) + ((a1[0] < 4u * (E + lpos0)) & (post.y < 1.0f));
                    else (void)post;
                }
                if (LDPC_VAR_PAIRS > 0 && (i / 2) % LDPC_VAR_PAIRS == LDPC_VAR_PAIRS - 1)
                    __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (VPT % 2 == 1) {
                constexpr int i = VPT - 1;
                uint32_t a0[DV];
                float cv[DV];
#pragma unroll
                for (int j = 0; j < DV; ++j) a0[j] = addr(i, j);
#pragma unroll
                for (int j = 0; j < DV; ++j) cv[j] = at(a0[j]);
                if constexpr (FINAL) {
                    float s = llr_log2(i);
#pragma unroll
                    for (int j = 0; j < DV; ++j) s += __builtin_amdgcn_logf(cv[j]);
                    if constexpr (!MC) pr[i] = s;
                } else {
                    const float post = edges(cv, L[i], [&](int j, float R) { at(a0[j]) = ratio_wire(R); });
                    if constexpr (ET) {
                        put_hard(i, post < 1.0f, a0);
                        if constexpr (!MC) {
                            float pq = cv[0];
#pragma unroll
                            for (int j = 1; j < DV; ++j) pq *= cv[j];
                            pr[i] = pq;
                        }
                    }
                    if constexpr (MC) errs += (a0[0] < 4u * (E + lpos0)) & (post < 1.0f);
                    else (void)post;
                }
            }
            return errs;
        };
        auto var_phase = [&](auto final_tag) {
            constexpr bool FINAL = decltype(final_tag)::value;
            int errs = 0;
            // variables i, i+1 on float2 (packed sums and differences)
#pragma unroll
            for (int i = 0; i + 1 < VPT; i += 2) {
                uint32_t a0[DV], a1[DV];
                float2 cv[DV];
                float2 s = make_float2(L[i], L[i + 1]);
#pragma unroll
                for (int j = 0; j < DV; ++j) {  // all addresses first: the gathers issue back to back
                    a0[j] = addr(i, j);
                    a1[j] = addr(i + 1, j);
                }
#pragma unroll
                for (int j = 0; j < DV; ++j) cv[j] = make_float2(at(a0[j]), at(a1[j]));
#pragma unroll
                for (int j = 0; j < DV; ++j) s = s + cv[j];
                if constexpr (!FINAL) {
#pragma unroll
                    for (int j = 0; j < DV; ++j) {
                        const float2 w = s - cv[j];  // min-sum (sum-product: var_phase_prod)
                        at(a0[j]) = w.x;
                        at(a1[j]) = w.y;
                    }
                }
                if constexpr (!MC) {
                    if (FINAL || ET) { pr[i] = s.x; pr[i + 1] = s.y; }
                }
                if constexpr (ET) {
                    put_hard(i, s.x < 0.0f, a0);
                    put_hard(i + 1, s.y < 0.0f, a1);
                }
                if constexpr (MC) errs += ((a0[0] < 4u * (E + lpos0)) & (s.x < 0.0f)) + ((a1[0] < 4u * (E + lpos0)) & (s.y < 0.0f));
                // LDPC_VAR_PAIRS pairs' gathers in flight per thread (VGPR budget of
                // 4 waves/SIMD; the CU's 16 waves hide LDS latency)
                if (LDPC_VAR_PAIRS > 0 && (i / 2) % LDPC_VAR_PAIRS == LDPC_VAR_PAIRS - 1)
                    __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (VPT % 2 == 1) {
                constexpr int i = VPT - 1;
                uint32_t a0[DV];
                float cv[DV];
                float s = L[i];
#pragma unroll
                for (int j = 0; j < DV; ++j) a0[j] = addr(i, j);
#pragma unroll
                for (int j = 0; j < DV; ++j) cv[j] = at(a0[j]);
#pragma unroll
                for (int j = 0; j < DV; ++j) s += cv[j];
                if constexpr (!FINAL) {
#pragma unroll
                    for (int j = 0; j < DV; ++j) at(a0[j]) = s - cv[j];
                }
                if constexpr (!MC) {
                    if (FINAL || ET) pr[i] = s;
                }
                if constexpr (ET) {
                    put_hard(i, s < 0.0f, a0);
                }
                if constexpr (MC) errs += (a0[0] < 4u * (E + lpos0)) & (s < 0.0f);
            }
            return errs;
        };

        int it = 0;
        for (; it < iters; ++it) {
            if (it > 0) __syncthreads();  // variable phase (msg, hs) complete
            // check phase; with ET it also evaluates the syndrome of the previous
            // iteration's hard decisions, and the decoder stops before the next
            // variable phase when every check is satisfied
            int unsat = 0;
#pragma unroll LDPC_CHECK_PAIRS_UNROLL
            for (int q = tid; q < npairs; q += T) {
                float2 *pp = reinterpret_cast<float2 *>(msg) + q * DC;
                if (ET && it > 0) {
                    // the pair's 2*DC decision bytes: even bytes check 2q, odd 2q+1
                    const uint32_t *hw = reinterpret_cast<const uint32_t *>(hs + q * 2 * DC);
                    uint32_t x = 0;
#pragma unroll
                    for (int w = 0; w < DC / 2; ++w) x ^= hw[w];
                    x ^= x >> 16;
                    unsat |= (x & 1) | (2 * q + 1 < m ? (x >> 8) & 1 : 0);
                }
                float2 x2[DC];
#pragma unroll
                for (int i = 0; i < DC; ++i) x2[i] = pp[i];
                if constexpr (ALGO == 0) {
                    check_update_spa_pair_rwire<DC>(x2);
                } else {
                    float xa[DC], xb[DC];
#pragma unroll
                    for (int i = 0; i < DC; ++i) { xa[i] = x2[i].x; xb[i] = x2[i].y; }
                    if constexpr (DC == 6) {
                        check_update_ms6(xa, a.alpha);
                        check_update_ms6(xb, a.alpha);
                    } else {
                        check_update<ALGO, DC>(xa, a.alpha);
                        check_update<ALGO, DC>(xb, a.alpha);
                    }
#pragma unroll
                    for (int i = 0; i < DC; ++i) x2[i] = make_float2(xa[i], xb[i]);
                }
#pragma unroll
                for (int i = 0; i < DC; ++i) pp[i] = x2[i];
            }
            if constexpr (ET) {
                if (!__syncthreads_or(unsat | (it == 0))) break;
            } else {
                __syncthreads();
            }
            // fixed-count decode: the last variable phase runs after the loop
            if (!ET && !MC && it == iters - 1) break;
            int errs = 0;
            {
                if constexpr (PROD) errs = var_phase_prod(std::false_type{});
                else errs = var_phase(std::false_type{});
            }
            hfirst = false;
            if (MC) {
                const int w = wave_sum(errs);
                if ((tid & (kWave - 1)) == 0) atomicAdd(&curve[it + 1], w);
            }
        }
        if (!ET && !MC && iters > 0) {
            if constexpr (PROD) (void)var_phase_prod(std::true_type{});
            else (void)var_phase(std::true_type{});
            it = iters;
        }
        if constexpr (PF) {
            const int bn = b + (int)gridDim.x;
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                const int v = tid + k * T;
                if (v < n && bn < a.B) nx[k] = a.llr[(size_t)bn * n + v];
            }
        }
        if constexpr (PROD && ET && !MC) {  // early stop: posterior = L + log2(prod r_j)
            if (iters > 0) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) pr[i] = llr_log2(i) + __builtin_amdgcn_logf(pr[i]);
            }
        }
        if constexpr (MC) {
            __syncthreads();
            int32_t *tr = a.trial + (size_t)b * (iters + 1);
            const int last = curve[it];
            for (int i = tid; i <= iters; i += T) tr[i] = i <= it ? curve[i] : last;
            if (tid == 0) a.its[b] = it;
        } else {
            // posteriors out through LDS (coalesced HBM writes)
            __syncthreads();
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int vv = a.lane_var[tid + i * T];
                if (vv >= 0) msg[vv] = pr[i];
            }
            __syncthreads();
            for (int v = tid; v < n; v += T) {
                const float s = msg[v];
                if (a.post) a.post[(size_t)b * n + v] = s * Domain<ALGO>::out;
                if (a.hard) a.hard[(size_t)b * n + v] = (uint8_t)(s < 0.0f);
            }
            if (a.its && tid == 0) a.its[b] = it;
        }
    }
}

// The instantiations: the rows of the shape table (kernel_shapes.hpp), from which lds_shape gives
// the lane layout its (T, VPT)
template <int ALGO, bool ET, bool MC>
hipError_t launch_lds36_modes(const BpPlan &p, const ldpc_graph &g, BpArgs a, hipStream_t s) {
    a.lane_var = g.lane_var;
    a.lane_slot = g.lane_slot;
    a.E = lds_pair_span(g.m, 6);  // message positions (lds_pair_pos), dummies after
#define LDPC_ROW(T, VPT)                      \
    if (g.lane_T == T && g.lane_VPT == VPT) \
        return launch_lds(bp_lds_kernel<3, 6, T, VPT, ALGO, ET, MC>, dim3(p.grid), dim3(T), p.lds, s, a);
    LDPC_LDS36_SHAPES(LDPC_ROW)
#undef LDPC_ROW
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_lds36(const BpPlan &p, const ldpc_graph &g, BpArgs a, int algo, bool et, bool mc, hipStream_t s) {
    return bp_modes(algo, et, mc, [&](auto A, auto E, auto M) {
        return launch_lds36_modes<decltype(A)::value, decltype(E)::value, decltype(M)::value>(p, g, a, s);
    });
}

}  // namespace ldpc
