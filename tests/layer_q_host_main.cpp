// Stand-alone driver of the host-only code behind the fixed-point layered decoder (the layer
// schedule's tables and the per-layer check base of csrc/graph_host.cpp, bp_layer_q_plan of
// csrc/bp_plan.cpp), built by tests/test_layer_q_host.py under AddressSanitizer and
// UndefinedBehaviorSanitizer and linked against no HIP library.
//   layer_q_host_main GRAPH   GRAPH: int32 n, m, E, check_ptr[m+1], check_var[E], var_ptr[n+1], var_slot[E]
// Prints "key=value" words: the schedule's scalars, the check base (','-separated), whether the
// tables agree with each other, and the plans of a handful of calls (fields ':'-, plans ';'-separated).
#include <cstdio>
#include <string>
#include <vector>

#include "graph_host.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {
void set_error(const std::string &msg) { fprintf(stderr, "error: %s\n", msg.c_str()); }
}  // namespace ldpc

using namespace ldpc;

// B, iters, algo, early_stop, mc, want_post: CALLS of tests/test_layer_q_host.py
static const int kCalls[][6] = {{24, 20, 1, 0, 0, 1}, {128, 20, 1, 1, 1, 0}, {300, 50, 1, 1, 0, 0}, {128, 40000, 1, 1, 1, 0}};

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    int32_t hdr[3];
    if (!f || fread(hdr, 4, 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] <= 0) return 2;
    const int n = hdr[0], m = hdr[1], E = hdr[2];
    std::vector<int32_t> cptr(m + 1), cvar(E), vptr(n + 1), vslot(E);
    for (std::vector<int32_t> *a : {&cptr, &cvar, &vptr, &vslot})
        if (fread(a->data(), 4, a->size(), f) != a->size()) return 2;
    fclose(f);

    HostGraph h;
    if (host_graph_from_csr(cptr.data(), cvar.data(), vptr.data(), vslot.data(), n, m, h) != LDPC_OK) return 3;
    GraphShape g;
    HostLayouts L;
    host_layouts(h, g, L);
    const LayerSchedule &S = L.lay;
    printf("n=%d m=%d E=%d max_cdeg=%d lay_L=%d lay_max=%d\n", g.n, g.m, g.E, g.max_cdeg, g.lay_L, g.lay_max);
    std::string base;
    for (int32_t b : S.ptr) base += std::string(base.empty() ? "" : ",") + std::to_string(b);
    printf("cbase=%s\n", base.empty() ? "-" : base.c_str());
    // the record of the check at position p of layer l is cbase[l] + p: it must be the check the
    // layer's tables put there (its first variable, and its degree from the rows' widths)
    bool ok = (int)S.ptr.size() == S.L + 1 && (S.L == 0 || S.ptr[S.L] == m);
    for (int l = 0; ok && l < S.L; ++l) {
        const int32_t *row = &S.tab[(size_t)l * kLayerTab];
        ok = row[1] - row[0] == S.ptr[l + 1] - S.ptr[l];
        for (int p = 0; ok && p < S.ptr[l + 1] - S.ptr[l]; ++p) {
            const int c = S.chk[S.ptr[l] + p], d = h.cptr[c + 1] - h.cptr[c];
            for (int j = 0; ok && j < kLayerMaxD; ++j) {
                const bool has = p < row[j + 1] - row[j];
                ok = has == (j < d) && (!has || S.var[row[j] + p] == h.cvar[h.cptr[c] + j]);
            }
        }
    }
    printf("tables_agree=%d\n", (int)ok);
    std::string plans;
    for (const auto &c : kCalls) {
        const BpPlan p = bp_layer_q_plan(g, c[0], c[1], c[2], c[3] != 0, c[4] != 0, c[5] != 0, 256);
        plans += std::string(plans.empty() ? "" : ";") + p.name + ":" + std::to_string((int)p.path) + ":" +
                 std::to_string(p.threads) + ":" + std::to_string(p.grid) + ":" + std::to_string(p.lds) + ":" +
                 std::to_string(p.wg_per_cu) + ":" + std::to_string(p.scratch);
    }
    printf("plans=%s\n", plans.c_str());
    return 0;
}
