// The launch plan of a BEC erasure-decoding call: which kernel runs, its workgroup shape, grid
// and LDS.  Host-only and pure (no HIP call, no environment): bec.hip and peel.hip launch what it
// says, tests/test_bec_plan.py reads it through ldpc_debug_bec_plan without a device.
#include "ldpc_internal.hpp"

// Compile-time switches of the selection (scripts/build_kernel_variant.sh)
#ifndef LDPC_BEC_BITS
#define LDPC_BEC_BITS 1  // fixed-code BEC Monte-Carlo on the bit-sliced kernel when its planes fit LDS
#endif
#ifndef LDPC_BEC_DEC_BITS
#define LDPC_BEC_DEC_BITS 1  // batch BEC decode (B >= 64) on the bit-sliced kernel when its planes fit LDS
#endif
#ifndef LDPC_ENS_PEEL
#define LDPC_ENS_PEEL 1  // ensemble MC on the frontier-peeling decoder (peel.hip) where it fits
#endif

namespace ldpc {
namespace {

// bec_kernel's carve (bec.hip, errs | mvc | cs): caller errors[] int32[iters] | word u8[n] | one byte per check
size_t word_lds(int n, int m, int iters) { return pad16((size_t)iters * 4) + pad16((size_t)n) + (size_t)m; }

// The bit-sliced kernels' carve (bec.hip; Ev | On | cnt | itsl | flag of bec_mc_bits_kernel,
// Xv | Xc | cnt | act | flag of bec_dec_bits_kernel): planes [n + m][W], then per codeword of the
// workgroup cnt + its (Mc, 8 bytes) or cnt alone (Decode, 4 bytes, and act[W]), then the flags.
// A plane byte carries 8 codewords under Mc, 4 under Decode (erased and value bits).
int bits_cw_per_wg(bool dec, int W, int plane) { return (dec ? 4 : 8) * plane * W; }
size_t bits_lds(int n, int m, bool dec, int W, int plane) {
    return pad16(((size_t)n + m) * W * plane) + (size_t)(dec ? 4 : 8) * bits_cw_per_wg(dec, W, plane) +
           (dec ? 4 * W : 0) + 16;
}

// bec_peel_kernel's carve (peel.hip, st | vf | fb | fl): check state u32[m] | erased-variable bits |
// frontier snapshot bits | two frontier lists u16[F]
size_t peel_lds(int n, int m, int F) {
    return (size_t)4 * (m + ((n + 31) >> 5) + ((m + 31) >> 5)) + (size_t)4 * F;
}

void word_plan(BecPlan &p, int n, int m, int B, int iters) {
    const size_t lds = word_lds(n, m, iters);
    if (lds > kBecWordLdsCap) return;
    const int T = n >= 4096 ? 1024 : 256;
    const auto *row = shapes::find(shapes::kBecWord, [&](const shapes::BecWord &r) { return r.T == T; });
    if (!row) return;  // not with these rules: both thread counts have their row
    p.kernel = BecKernel::Word;
    p.threads = T;
    p.cw_per_wg = 1;
    p.grid = B;
    p.lds = lds;
    p.cap = kBecWordLdsCap;
    p.name = row->name;
}

// Plane word (u32 x W words per variable, or u8 for graphs whose u32 planes do not fit) and
// workgroup size for this graph and batch; false when not even u8 planes fit.
bool bits_plan(BecPlan &p, int n, int m, int B, bool dec) {
    auto grid = [&](int W, int plane) {
        const int nb = bits_cw_per_wg(dec, W, plane);
        return ((int64_t)B + nb - 1) / nb;
    };
    int W = 1, plane = 4, T = n > 4096 ? 512 : 256;
    size_t cap = kBecBitsLdsCap;
    // wider planes while the workgroups still fill 256 CUs several times over, LDS for >= 2 per CU
    for (int w : {4, 2, 1})
        if (bits_lds(n, m, dec, w, 4) <= kBecBitsWideLdsCap && grid(w, 4) >= 1024) {
            W = w;
            cap = kBecBitsWideLdsCap;
            break;
        }
    if (bits_lds(n, m, dec, W, plane) > cap) {
        plane = 1;
        T = 1024;
        if (bits_lds(n, m, dec, W, plane) > cap) return false;
    }
    // the instantiation: the shape table's row (kernel_shapes.hpp, what bec.hip compiles).  Every
    // (T, W, plane) the rules above give has one; a shape without a row would be no plan
    // (BecKernel::None), not another kernel's.
    const auto *row = shapes::find(shapes::kBecBits, [&](const shapes::BecBits &r) {
        return r.T == T && r.W == W && r.plane == plane;
    });
    if (!row) return true;
    p.kernel = dec ? BecKernel::DecBits : BecKernel::McBits;
    p.threads = T;
    p.W = W;
    p.plane = plane;
    p.cw_per_wg = bits_cw_per_wg(dec, W, plane);
    p.grid = grid(W, plane);
    p.lds = bits_lds(n, m, dec, W, plane);
    p.cap = cap;
    p.name = dec ? row->dec : row->mc;
    return true;
}

// Regular (dv, dc) graphs whose check state fits LDS beside frontier lists of at least 256
// entries; the check word holds count << 24 | sum of ids (dc <= 255, dc n < 2^24), a list
// entry is a u16 check id (m <= 65,536).
bool peel_plan(BecPlan &p, int n, int m, int dc, int B, int peel_cap) {
    if (m > 65536 || dc > 255 || (long)dc * n >= (1L << 24) || peel_lds(n, m, 256) > kPeelLdsCap) return false;
    p.kernel = BecKernel::Peel;
    p.threads = 1024;
    p.cw_per_wg = 1;
    p.grid = B;
    p.F = (int)std::min<size_t>((size_t)m, (kPeelLdsCap - peel_lds(n, m, 0)) / 4);
    if (peel_cap > 0) p.F = std::min(p.F, peel_cap);
    p.lds = peel_lds(n, m, p.F);
    p.cap = kPeelLdsCap;
    p.name = "bec_peel_kernel<1024>";
    return true;
}

}  // namespace

BecPlan bec_plan(int n, int m, int dc, int B, int iters, BecMode mode, int peel_cap) {
    BecPlan p;
    bool bits = false;
    if (mode == BecMode::Mc) bits = LDPC_BEC_BITS;
    // a few words (the drop-in's B = 1): one workgroup per codeword
    if (mode == BecMode::Decode) bits = LDPC_BEC_DEC_BITS && B >= 64;
    if (bits && bits_plan(p, n, m, B, mode == BecMode::Decode)) return p;
    if (mode == BecMode::EnsMc && LDPC_ENS_PEEL && peel_plan(p, n, m, dc, B, peel_cap)) return p;
    word_plan(p, n, m, B, iters);
    return p;
}

}  // namespace ldpc
