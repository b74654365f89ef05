// Systematic encoder description of a Tanner graph (encode_host.cpp): the rank of H over GF(2), the
// information and parity positions, and the dense matrix that gives the parity bits from the
// information bits.  Host-only and pure like graph_host.cpp: no HIP call, no environment variable,
// so it links and runs without a device (tests/encode_host_main.cpp).
//
// H over GF(2): entry (c, v) is the parity of the number of slots of check c that hold v, so a
// variable a check holds twice cancels -- the XOR-over-slots syndrome the decoders compute.
//
// kEncodeRule, the elimination: bit-packed Gauss-Jordan on 64-bit words.  Columns are scanned from
// n - 1 downward; a column pivots on the lowest unused row that holds a 1 in it (a column without
// one is an information position), and the pivot row is added to every other row that holds a 1
// there.  The parity positions therefore sit at the high end of the word, in falling order
// (par_pos[0] is the largest), and the same graph always gives the same positions and the same A.
#pragma once
#include "graph_host.hpp"

namespace ldpc {

extern const char *const kEncodeRule;

struct EncoderDesc {
    int n = 0, rank = 0, K = 0;         // K = n - rank: the code's dimension (>= n - m)
    int KW = 0;                         // u32 words of a row of A: ceil(K / 32)
    std::vector<int32_t> info_pos;      // [K]    the non-pivot columns, ascending
    std::vector<int32_t> par_pos;       // [rank] the pivot columns, in pivot order (falling)
    // [rank][KW]: x[par_pos[i]] = XOR_j A[i][j] u[j], bit j of row i = bit (j & 31) of word j >> 5;
    // the bits from K up to 32 KW are zero
    std::vector<uint32_t> A;
};

// Reads h.n, h.m, h.cptr and h.cvar (validated by host_graph_from_*).  K = 0 is valid (the code is
// {0}); a variable in no check is an information position.
void build_encoder(const HostGraph &h, EncoderDesc &e);

// What the device holds (encode.hip): At [KW][rank], the transposed copy of A (word jw of every row
// side by side, so a wave's loads coalesce), and src [n]: j >= 0 for information position j,
// ~i < 0 for parity position i.
void encoder_device_tables(const EncoderDesc &e, std::vector<uint32_t> &At, std::vector<int32_t> &src);

}  // namespace ldpc
