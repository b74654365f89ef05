// Validation and packing of a rate-matching description (rate_match_host.hpp).  Host-only.
#include "rate_match_host.hpp"

#include <string>

#include "errors.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {

int rate_match_pack(int n, const uint8_t *cls, const uint8_t *count, RateMatchDesc &d) {
    LDPC_REQUIRE(n >= 1, "rate matching: n must be >= 1");
    LDPC_REQUIRE(cls, "rate matching: null class array");
    d = RateMatchDesc();
    d.n = n;
    d.packed.assign(4 * (((size_t)n + 3) / 4), (uint8_t)LDPC_RM_PUNCT);
    for (int v = 0; v < n; ++v) {
        if (cls[v] > LDPC_RM_KNOWN) {
            set_error("rate matching: class of variable " + std::to_string(v) + " is " + std::to_string(cls[v]) +
                      " (LDPC_RM_TX 0, LDPC_RM_PUNCT 1, LDPC_RM_KNOWN 2)");
            return LDPC_EINVAL;
        }
        if (count && count[v] > 1) {
            set_error("rate matching: count mask of variable " + std::to_string(v) + " is " +
                      std::to_string(count[v]) + " (0 or 1)");
            return LDPC_EINVAL;
        }
        const uint8_t c = count ? count[v] : (uint8_t)(cls[v] != LDPC_RM_KNOWN);
        d.packed[v] = (uint8_t)(cls[v] | c << 2);
        d.n_tx += cls[v] == LDPC_RM_TX;
        d.n_punct += cls[v] == LDPC_RM_PUNCT;
        d.n_known += cls[v] == LDPC_RM_KNOWN;
        d.n_count += c;
    }
    return LDPC_OK;
}

}  // namespace ldpc
