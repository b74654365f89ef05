// Rate-matching description of a length-n code (rate_match_host.cpp): validation and the packed
// device form.  Host-only and pure like encode_host.cpp: no HIP call, no environment variable, so
// ldpc_debug_rate_match_pack runs without a device.  The semantics are include/ldpc_mi355x.h's.
#pragma once
#include <stdint.h>

#include <vector>

namespace ldpc {

struct RateMatchDesc {
    int n = 0, n_tx = 0, n_punct = 0, n_known = 0, n_count = 0;
    // [4 ceil(n / 4)]: byte v = cls[v] | count[v] << 2; the padding bytes are LDPC_RM_PUNCT,
    // uncounted (1), so a dword of padding-only or padding-and-untransmitted positions draws nothing
    std::vector<uint8_t> packed;
};

// cls [n] in {0, 1, 2}; count [n] in {0, 1}, or nullptr for the default (1 where cls != LDPC_RM_KNOWN).
// LDPC_OK, or LDPC_EINVAL with the error text set.
int rate_match_pack(int n, const uint8_t *cls, const uint8_t *count, RateMatchDesc &d);

}  // namespace ldpc
