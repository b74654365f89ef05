// Stand-alone driver of the host-only graph preparation (csrc/graph_host.cpp, loc_layout.cpp,
// bp_plan.cpp), built by tests/test_host_layouts.py under AddressSanitizer and
// UndefinedBehaviorSanitizer and linked against no HIP library.
//   host_layouts_main GRAPH   GRAPH: int32 n, m, E, check_ptr[m+1], check_var[E], var_ptr[n+1], var_slot[E]
// Prints "key=value" words: the shape scalars with default options, with the local-edge layout
// off (off_*), and the launch plans of a handful of calls (names ';'-separated).
#include <cstdio>
#include <string>
#include <vector>

#include "graph_host.hpp"
#include "ldpc_mi355x.h"

namespace ldpc {
void set_error(const std::string &msg) { fprintf(stderr, "error: %s\n", msg.c_str()); }
}  // namespace ldpc

using namespace ldpc;

// B, iters, algo, early_stop, mc, want_post: PLAN_CALLS of tests/test_host_layouts.py
static const int kCalls[][6] = {{300, 50, 0, 0, 0, 1},   {300, 50, 1, 0, 0, 1}, {300, 50, 0, 1, 0, 0},
                                {70000, 50, 0, 1, 0, 1}, {300, 50, 1, 1, 1, 0}, {300, 600, 0, 0, 1, 0}};

static void print_plans(const GraphShape &g, const char *key, bool scratch) {
    std::string names, bytes;
    for (const auto &c : kCalls) {
        const BpPlan p = bp_plan(g, c[0], c[1], c[2], c[3] != 0, c[4] != 0, c[5] != 0, 256);
        names += std::string(names.empty() ? "" : ";") + p.name;
        bytes += std::string(bytes.empty() ? "" : ",") + std::to_string(p.scratch);
    }
    printf("%s=%s\n", key, names.c_str());
    if (scratch) printf("scratch=%s\n", bytes.c_str());
}

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
    printf("n=%d m=%d E=%d consistent=%d max_vdeg=%d max_cdeg=%d\n", g.n, g.m, g.E, (int)g.consistent, g.max_vdeg,
           g.max_cdeg);
    printf("lane_T=%d lane_VPT=%d lane_len=%zu\n", g.lane_T, g.lane_VPT, L.lane_var.size());
    printf("irr_VPT=%d irr_KC=%d irr_DC=%d irr_S=%d irr_P=%d irr_len=%zu\n", g.irr_VPT, g.irr_KC, g.irr_DC, g.irr_S,
           g.irr_P, L.irr_lane.size());
    printf("loc_T=%d loc_KP=%d loc_DVN=%d loc_P=%d loc_words=%d loc_ncls=%d loc_dvn0=%d loc_dvn1=%d\n", g.loc_T,
           g.loc_KP, g.loc_DVN, g.loc_P, g.loc_words, g.loc_ncls, g.loc_dvn0, g.loc_dvn1);
    printf("variant=%d\n", loc_variant(g));
    print_plans(g, "plans", true);

    LayoutOptions off;
    off.loc_layout = false;
    GraphShape g0;
    HostLayouts L0;
    host_layouts(h, g0, L0, true, off);
    printf("off_lane_T=%d off_irr_VPT=%d off_loc_KP=%d\n", g0.lane_T, g0.irr_VPT, g0.loc_KP);
    print_plans(g0, "off_plans", false);
    return 0;
}
