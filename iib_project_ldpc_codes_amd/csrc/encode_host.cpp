// The systematic encoder description: see encode_host.hpp (H over GF(2), kEncodeRule).
#include "encode_host.hpp"

namespace ldpc {

const char *const kEncodeRule = "gauss-jordan/columns-descending/lowest-unused-row/v1";

void build_encoder(const HostGraph &h, EncoderDesc &e) {
    const int n = h.n, m = h.m;
    const size_t W = ((size_t)n + 63) / 64;  // 64-bit words of a row of H
    std::vector<uint64_t> H((size_t)m * W, 0);
    for (int c = 0; c < m; ++c)
        for (int s = h.cptr[c]; s < h.cptr[c + 1]; ++s) {
            const int v = h.cvar[s];
            H[(size_t)c * W + (v >> 6)] ^= (uint64_t)1 << (v & 63);
        }
    std::vector<char> used(m, 0), pivot_col(n, 0);
    std::vector<int32_t> pivot_row;
    e = EncoderDesc();
    e.n = n;
    for (int col = n - 1; col >= 0; --col) {
        const size_t w = (size_t)col >> 6;
        const uint64_t bit = (uint64_t)1 << (col & 63);
        int p = -1;
        for (int r = 0; r < m; ++r)
            if (!used[r] && (H[(size_t)r * W + w] & bit)) {
                p = r;
                break;
            }
        if (p < 0) continue;
        used[p] = 1;
        pivot_col[col] = 1;
        pivot_row.push_back(p);
        e.par_pos.push_back(col);
        const uint64_t *src = &H[(size_t)p * W];
        for (int r = 0; r < m; ++r) {
            if (r == p || !(H[(size_t)r * W + w] & bit)) continue;
            uint64_t *dst = &H[(size_t)r * W];
            for (size_t i = 0; i < W; ++i) dst[i] ^= src[i];
        }
    }
    e.rank = (int)e.par_pos.size();
    e.K = n - e.rank;
    e.KW = (e.K + 31) / 32;
    e.info_pos.reserve(e.K);
    for (int v = 0; v < n; ++v)
        if (!pivot_col[v]) e.info_pos.push_back(v);
    // Row i of A: the pivot row's bits at the information positions (its other pivot columns are 0)
    e.A.assign((size_t)e.rank * e.KW, 0u);
    for (int i = 0; i < e.rank; ++i) {
        const uint64_t *row = &H[(size_t)pivot_row[i] * W];
        uint32_t *a = e.A.data() + (size_t)i * e.KW;
        for (int j = 0; j < e.K; ++j) {
            const int v = e.info_pos[j];
            a[j >> 5] |= (uint32_t)(row[v >> 6] >> (v & 63) & 1u) << (j & 31);
        }
    }
}

void encoder_device_tables(const EncoderDesc &e, std::vector<uint32_t> &At, std::vector<int32_t> &src) {
    At.assign((size_t)e.KW * e.rank, 0u);
    for (int i = 0; i < e.rank; ++i)
        for (int jw = 0; jw < e.KW; ++jw) At[(size_t)jw * e.rank + i] = e.A[(size_t)i * e.KW + jw];
    src.assign(e.n, 0);
    for (int j = 0; j < e.K; ++j) src[e.info_pos[j]] = j;
    for (int i = 0; i < e.rank; ++i) src[e.par_pos[i]] = ~i;
}

}  // namespace ldpc
