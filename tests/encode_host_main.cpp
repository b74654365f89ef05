// Stand-alone driver of the host-only code behind the encoder (the elimination and the device tables
// of csrc/encode_host.cpp, encode_plan of csrc/encode_plan.cpp), built by
// tests/test_encode_host_san.py under AddressSanitizer and UndefinedBehaviorSanitizer and linked
// against no HIP library.
//   encode_host_main GRAPH   GRAPH: int32 n, m, E, check_ptr[m+1], check_var[E]
// Prints "key=value" words: rank and K, the positions and the words of A (','-separated, "-" when
// empty), whether the device tables agree with the description, and the plans of a few batch sizes
// (fields ':'-, plans ';'-separated).
#include <cstdio>
#include <string>
#include <vector>

#include "encode_host.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {
void set_error(const std::string &msg) { fprintf(stderr, "error: %s\n", msg.c_str()); }
}  // namespace ldpc

using namespace ldpc;

static const int kBatches[] = {1, 33, 257, 65536};  // BATCHES of tests/test_encode_host_san.py

template <typename T>
static void print_list(const char *key, const std::vector<T> &a) {
    std::string s;
    for (T x : a) s += std::string(s.empty() ? "" : ",") + std::to_string((unsigned long)x);
    printf("%s=%s\n", key, s.empty() ? "-" : s.c_str());
}

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    int32_t hdr[3];
    if (!f || fread(hdr, 4, 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] < 0) return 2;
    HostGraph h;
    h.n = hdr[0], h.m = hdr[1];
    h.cptr.resize((size_t)h.m + 1);
    h.cvar.resize(hdr[2]);
    for (std::vector<int32_t> *a : {&h.cptr, &h.cvar})
        if (fread(a->data(), 4, a->size(), f) != a->size()) return 2;
    fclose(f);

    EncoderDesc e;
    build_encoder(h, e);
    printf("n=%d rank=%d K=%d KW=%d\n", e.n, e.rank, e.K, e.KW);
    print_list("info", e.info_pos);
    print_list("par", e.par_pos);
    print_list("A", e.A);

    std::vector<uint32_t> At;
    std::vector<int32_t> src;
    encoder_device_tables(e, At, src);
    bool ok = At.size() == e.A.size() && (int)src.size() == e.n;
    for (int i = 0; ok && i < e.rank; ++i)
        for (int jw = 0; ok && jw < e.KW; ++jw) ok = At[(size_t)jw * e.rank + i] == e.A[(size_t)i * e.KW + jw];
    for (int v = 0; ok && v < e.n; ++v) {
        const int s = src[v];
        ok = s >= 0 ? (s < e.K && e.info_pos[s] == v) : (~s < e.rank && e.par_pos[~s] == v);
    }
    printf("tables_agree=%d\n", ok ? 1 : 0);

    std::string plans;
    for (int B : kBatches) {
        const EncodePlan p = encode_plan(e.n, e.K, e.rank, B);
        plans += std::string(plans.empty() ? "" : ";") + p.name + ":" + std::to_string(p.threads) + ":" +
                 std::to_string(p.W) + ":" + std::to_string(p.grid) + ":" + std::to_string(p.lds) + ":" +
                 std::to_string(p.scratch) + ":" + std::to_string(p.write_grid);
    }
    printf("plans=%s\n", plans.c_str());
    return 0;
}
