// The shape tables: for each kernel family whose launch plan picks among template instantiations,
// the one list of the instantiations that exist.  The host-only plans (*_plan.cpp, lds_shape,
// loc_variant) select a row and take the display name from it; the launchers (the .hip files)
// expand the same list into their instantiations, so a shape that the plan can name is a shape
// that is compiled, and the other way round.  Plain C++ (the plans are also built without hipcc).
//
// A row is X(template arguments..., name tags...).  The rows are in the order in which the
// launchers instantiate, which is the order of the kernels in the code object: it is kept as it
// was measured, so a new row goes to the end of its list.
#pragma once
#include <stdint.h>

// bec_dec_bits_kernel / bec_mc_bits_kernel (bec.hip): threads, plane words per variable, plane word, its tag
#define LDPC_BEC_BITS_SHAPES(X)                                                                           \
    X(1024, 1, uint8_t, u8) X(256, 4, uint32_t, u32) X(256, 2, uint32_t, u32) X(256, 1, uint32_t, u32)   \
    X(512, 4, uint32_t, u32) X(512, 2, uint32_t, u32) X(512, 1, uint32_t, u32)
// bec_kernel (bec.hip): threads
#define LDPC_BEC_WORD_SHAPES(X) X(1024) X(256)
// gb_kernel (gb.hip): threads, plane word, its tag; each in the four (early stop, Monte-Carlo) modes
#define LDPC_GB_SHAPES(X) X(256, uint32_t, u32) X(1024, uint32_t, u32) X(1024, uint16_t, u16) X(1024, uint8_t, u8)
// encode_parity_kernel (encode.hip): plane words of 32 codewords per workgroup
#define LDPC_ENC_TILES(X) X(4) X(2) X(1)
// bp_lds_kernel<3,6> (bp_lds.hip): threads, variables per thread, rising per thread count.  No plan
// reaches (1024, 2) at the shipped LDPC_LDS_SPARE -- 256 x 9 lanes cover every n <= 2048, and
// n = 2049 already needs 2,090 -- but the row stays: the code object must not change.
#define LDPC_LDS36_SHAPES(X)                                                          \
    X(256, 1) X(256, 2) X(256, 3) X(256, 5) X(256, 9)                                 \
    X(1024, 2) X(1024, 3) X(1024, 5) X(1024, 6) X(1024, 9) X(1024, 10) X(1024, 11) X(1024, 14)
// bp_loc_kernel (bp_loc.hpp): threads, check pairs per thread.  Both variants (LocVariant) have
// the common rows; the 512-thread rows are one variant's each (kLocReg36: two workgroups per CU;
// kLocRsu: 2 waves per SIMD).
#define LDPC_LOC_SHAPES(X) X(256, 1) X(256, 2) X(256, 3) X(256, 4) X(1024, 2) X(1024, 3)
#define LDPC_LOC_REG36_SHAPES(X) X(512, 5)
#define LDPC_LOC_RSU_SHAPES(X) X(512, 8) X(512, 10)
// bp_loc_chain_kernel<KP, T, TQ> (bp_loc_chain.hpp): the widths Tq = n / 20 of the chained layout that have an instantiation
// of their own, with Tq a compile-time constant.  500: n = 10,000, the benchmark's code.  A width is added for a
// code that is decoded for long (each row is another 128-VGPR kernel to compile); every other Tq runs the generic one.
#define LDPC_LOC_CHAIN_TQ(X) X(500)
// sample_regular_kernel (sampler.hip): buckets (= threads), permutation entry, its tag, the
// permutation in LDS, that as a tag
#define LDPC_SAMPLE_LEVEL_SHAPES(X) \
    X(256, uint16_t, u16, true, lds) X(512, uint16_t, u16, true, lds) X(1024, int32_t, int32, false, gmem)
// sample_seq_kernel and sample_search_kernel (sampler.hip): CSR degree structure, its tag, ring entry, its tag
#define LDPC_SAMPLE_SEQ_SHAPES(X) \
    X(true, csr, uint16_t, u16) X(true, csr, int, int) X(false, regular, uint16_t, u16) X(false, regular, int, int)
// sample_var_side_kernel (sampler.hip): threads, staged row entry, its tag
#define LDPC_SAMPLE_VAR_SIDE_SHAPES(X) X(1024, uint16_t, u16) X(1024, int32_t, int32)
// bp_qc_q_kernel (bp_qc_q.hip): threads, widest block-row degree; each in the four (early stop,
// Monte-Carlo) modes.  Row i is BpPath::QcQ64x8 + i (ldpc_internal.hpp lists them in this order).
#define LDPC_QC_Q_SHAPES(X) X(64, 8) X(64, 16) X(64, 32) X(256, 8) X(256, 16) X(256, 32)

namespace ldpc {
namespace shapes {

// The tables as data, for the plans: what a plan matches a row by, and the row's display names.
struct BecBits { int T, W, plane; const char *dec, *mc; };
struct BecWord { int T; const char *name; };
struct Gb { int T, plane; const char *name[2][2]; };  // [early stop][Monte-Carlo]
struct EncTile { int W; const char *name; };
struct Shape2 { int T, per_thread; };  // bp_lds: VPT; bp_loc: KP
struct SampleLevel { int K; bool lds; const char *name; };
struct SampleSeq { bool csr; int ring; const char *seq, *search; };
struct SampleVarSide { int T, row; const char *name; };
struct QcQ { int T, maxdc; const char *name; };

#define LDPC_ROW(T, W, P, TAG) \
    {T, W, (int)sizeof(P), "bec_dec_bits_kernel<" #T "," #W "," #TAG ">", "bec_mc_bits_kernel<" #T "," #W "," #TAG ">"},
constexpr BecBits kBecBits[] = {LDPC_BEC_BITS_SHAPES(LDPC_ROW)};
#undef LDPC_ROW
#define LDPC_ROW(T) {T, "bec_kernel<" #T ">"},
constexpr BecWord kBecWord[] = {LDPC_BEC_WORD_SHAPES(LDPC_ROW)};
#undef LDPC_ROW
#define LDPC_GB_NAME(T, TAG, MODES) "gb_kernel<" #T "," #TAG MODES ">"
#define LDPC_ROW(T, P, TAG)                                                    \
    {T, (int)sizeof(P), {{LDPC_GB_NAME(T, TAG, ""), LDPC_GB_NAME(T, TAG, ",mc")}, \
                         {LDPC_GB_NAME(T, TAG, ",es"), LDPC_GB_NAME(T, TAG, ",es,mc")}}},
constexpr Gb kGb[] = {LDPC_GB_SHAPES(LDPC_ROW)};
#undef LDPC_ROW
#undef LDPC_GB_NAME
#define LDPC_ROW(W) {W, "encode_parity_kernel<" #W ">"},
constexpr EncTile kEncTiles[] = {LDPC_ENC_TILES(LDPC_ROW)};
#undef LDPC_ROW
#define LDPC_ROW(T, N) {T, N},
constexpr Shape2 kLds36[] = {LDPC_LDS36_SHAPES(LDPC_ROW)};
constexpr Shape2 kLocReg36[] = {LDPC_LOC_SHAPES(LDPC_ROW) LDPC_LOC_REG36_SHAPES(LDPC_ROW)};
constexpr Shape2 kLocRsu[] = {LDPC_LOC_SHAPES(LDPC_ROW) LDPC_LOC_RSU_SHAPES(LDPC_ROW)};
#undef LDPC_ROW
#define LDPC_ROW(TQ) TQ,
constexpr int kLocChainTq[] = {LDPC_LOC_CHAIN_TQ(LDPC_ROW)};
#undef LDPC_ROW
#define LDPC_ROW(K, IDX, TAG, LDSBUF, MEM) {K, LDSBUF, "sample_regular_kernel<" #K "," #TAG "," #MEM ">"},
constexpr SampleLevel kSampleLevel[] = {LDPC_SAMPLE_LEVEL_SHAPES(LDPC_ROW)};
#undef LDPC_ROW
#define LDPC_ROW(CSR, FORM, IDX, TAG) \
    {CSR, (int)sizeof(IDX), "sample_seq_kernel<" #FORM "," #TAG ">", "sample_search_kernel<" #FORM "," #TAG ">"},
constexpr SampleSeq kSampleSeq[] = {LDPC_SAMPLE_SEQ_SHAPES(LDPC_ROW)};
#undef LDPC_ROW
#define LDPC_ROW(T, IDX, TAG) {T, (int)sizeof(IDX), "sample_var_side_kernel<" #T "," #TAG ">"},
constexpr SampleVarSide kSampleVarSide[] = {LDPC_SAMPLE_VAR_SIDE_SHAPES(LDPC_ROW)};
#undef LDPC_ROW
#define LDPC_ROW(T, D) {T, D, "bp_qc_q_kernel<" #T "," #D ">"},
constexpr QcQ kQcQ[] = {LDPC_QC_Q_SHAPES(LDPC_ROW)};
#undef LDPC_ROW

// The first row of `rows` that `match` accepts, nullptr when there is none
template <typename Row, int N, typename F>
const Row *find(const Row (&rows)[N], F match) {
    for (const Row &r : rows)
        if (match(r)) return &r;
    return nullptr;
}

}  // namespace shapes
}  // namespace ldpc
