// Stand-alone driver of the host-only code behind quasi-cyclic codes (the expansion, the block-row
// schedule through layer_tables and the row table of csrc/graph_host.cpp, bp_layer_q_plan's route
// of csrc/bp_plan.cpp), built by tests/test_qc_host_san.py under AddressSanitizer and
// UndefinedBehaviorSanitizer and linked against no HIP library.
//   qc_host_main BASE [table]   BASE: int32 mb, nb, Z, base[mb][nb]; "table": LayoutOptions::qc_kernel off
// Prints "key=value" words: the shape's scalars, the four CSR arrays and layer[] (','-separated),
// the check base, whether the schedule's tables and the row table agree with the expansion, and
// the plans of a handful of calls (fields ':'-, plans ';'-separated).  A refused base: "refused=1".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "graph_host.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {
void set_error(const std::string &msg) { fprintf(stderr, "error: %s\n", msg.c_str()); }
}  // namespace ldpc

using namespace ldpc;

// B, iters, algo, early_stop, mc, want_post: CALLS of tests/test_qc_host_san.py
static const int kCalls[][6] = {{24, 20, 1, 0, 0, 1}, {128, 20, 1, 1, 1, 0}, {300, 50, 1, 1, 0, 0}, {128, 40000, 1, 1, 1, 0}};

static void print_list(const char *key, const std::vector<int32_t> &a) {
    std::string s;
    for (int32_t x : a) s += std::string(s.empty() ? "" : ",") + std::to_string(x);
    printf("%s=%s\n", key, s.empty() ? "-" : s.c_str());
}

int main(int argc, char **argv) {
    FILE *f = argc >= 2 ? fopen(argv[1], "rb") : nullptr;
    int32_t hdr[3];
    if (!f || fread(hdr, 4, 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0) return 2;
    const int mb = hdr[0], nb = hdr[1], Z = hdr[2];
    std::vector<int32_t> base((size_t)mb * nb);
    if (fread(base.data(), 4, base.size(), f) != base.size()) return 2;
    fclose(f);

    HostGraph h;
    QcCode qc;
    if (host_graph_from_qc(mb, nb, Z, base.data(), h, qc) != LDPC_OK) {
        printf("refused=1\n");
        return 0;
    }
    GraphShape g;
    HostLayouts L;
    LayoutOptions opt;
    opt.qc = &qc;
    opt.qc_kernel = !(argc >= 3 && !strcmp(argv[2], "table"));
    host_layouts(h, g, L, true, opt);
    const LayerSchedule &S = L.lay;
    printf("n=%d m=%d E=%d max_cdeg=%d lay_L=%d lay_max=%d block_rows=%d qc_Z=%d qc_mb=%d qc_nb=%d\n", g.n, g.m, g.E,
           g.max_cdeg, g.lay_L, g.lay_max, (int)g.lay_block_rows, g.qc_Z, g.qc_mb, g.qc_nb);
    print_list("cptr", h.cptr);
    print_list("cvar", h.cvar);
    print_list("vptr", h.vptr);
    print_list("vslot", h.vslot);
    print_list("layer", S.layer);
    print_list("cbase", S.ptr);
    // the tables of the block-row schedule: position p of layer l is check l Z + p, with its
    // variables in slot order; the row table gives the same variables by the convention
    bool ok = S.L == mb && (int)S.ptr.size() == mb + 1 && (int)S.chk.size() == g.m;
    for (int l = 0; ok && l < S.L; ++l) {
        const int32_t *row = &S.tab[(size_t)l * kLayerTab];
        ok = S.ptr[l] == l * Z && row[1] - row[0] == Z;
        for (int p = 0; ok && p < Z; ++p) {
            const int c = l * Z + p, d = h.cptr[c + 1] - h.cptr[c];
            ok = S.chk[S.ptr[l] + p] == c;
            for (int j = 0; ok && j < kLayerMaxD; ++j) {
                const bool has = p < row[j + 1] - row[j];
                ok = has == (j < d) && (!has || S.var[row[j] + p] == h.cvar[h.cptr[c] + j]);
            }
        }
    }
    printf("tables_agree=%d\n", (int)ok);
    bool rok = (int)qc.row.size() == mb * kQcRow && (L.qc_row.empty() || L.qc_row == qc.row) &&
               L.qc_row.empty() == (g.qc_Z == 0);
    for (int r = 0; rok && r < mb; ++r) {
        const int32_t *row = &qc.row[(size_t)r * kQcRow];
        for (int i = 0; rok && i < Z; ++i) {
            const int c = r * Z + i;
            rok = row[0] == h.cptr[c + 1] - h.cptr[c];
            for (int j = 0; rok && j < kLayerMaxD; ++j) {
                const int t = i + row[2 + 2 * j], v = row[1 + 2 * j] + t - (t >= Z ? Z : 0);  // the kernel's form
                rok = j < row[0] ? v == h.cvar[h.cptr[c] + j] : (row[1 + 2 * j] == 0 && row[2 + 2 * j] == 0);
            }
        }
    }
    printf("row_table_agrees=%d\n", (int)rok);
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
