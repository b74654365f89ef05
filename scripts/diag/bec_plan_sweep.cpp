// bec_plan (csrc/bec_plan.cpp) over the sweep of tests/test_bec_plan.py, as a stand-alone host
// program for the sanitizers: it links the plan file alone (no HIP runtime, nothing preloaded).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Iiib_project_ldpc_codes_amd/csrc \
//       scripts/diag/bec_plan_sweep.cpp iib_project_ldpc_codes_amd/csrc/bec_plan.cpp -o bec_plan_sweep
// Exit status 0 and one summary line when every plan keeps its own bounds.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ldpc_internal.hpp"

int main() {
    struct Shape { int n, m, dc; };
    std::vector<Shape> shapes;
    for (int n = 64; n < 9000; n += 331) shapes.push_back({n, n / 2, 6});
    for (int n = 20000; n <= 120000; n += 500) shapes.push_back({n, n / 2, 6});
    for (int n = 4077; n < 150000; n += 2997) shapes.push_back({n, n / 9, 27});
    shapes.push_back({4104, 456, 27});
    shapes.push_back({4104, 228, 54});
    shapes.push_back({1, 1, 0});
    shapes.push_back({INT_MAX / 2, INT_MAX / 4, 255});
    const int batches[] = {0, 1, 63, 64, 66, 40000, 70000, 140000, INT_MAX};
    const int iters[] = {0, 5, 50, 1000, INT_MAX / 4};
    const int caps[] = {0, 8, INT_MAX};
    long plans = 0, none = 0, bad = 0;
    for (const Shape &s : shapes)
        for (int mode = 0; mode < 3; ++mode)
            for (int B : batches)
                for (int it : iters)
                    for (int cap : caps) {
                        const ldpc::BecPlan p = ldpc::bec_plan(s.n, s.m, s.dc, B, it, static_cast<ldpc::BecMode>(mode), cap);
                        ++plans;
                        if (p.kernel == ldpc::BecKernel::None) {
                            ++none;
                            continue;
                        }
                        const bool ok = p.lds <= p.cap && p.cap <= kLdsMax && p.threads >= 256 && p.threads <= 1024 &&
                                        p.cw_per_wg >= 1 && p.grid * p.cw_per_wg >= B && strlen(p.name) > 4 && strlen(p.name) < 64 &&
                                        (p.kernel != ldpc::BecKernel::Peel || (p.F >= 1 && p.F <= s.m));
                        if (!ok) {
                            ++bad;
                            fprintf(stderr, "bad plan: n %d m %d dc %d mode %d B %d iters %d cap %d -> %s\n", s.n, s.m, s.dc,
                                    mode, B, it, cap, p.name);
                        }
                    }
    printf("bec_plan sweep: %ld plans, %ld without a kernel, %ld out of bounds\n", plans, none, bad);
    return bad ? 1 : 0;
}
