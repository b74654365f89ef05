// Two facts bp_loc_kernel's fixed-count path rests on, checked on the device:
//  1. exp2(clamp(x, +-23)) == clamp(exp2(clamp(x, +-126)), 2^-23, 2^23) to the bit, for every
//     non-NaN float x (v_exp_f32 monotone and exact at +-23): the staging forms the wire value
//     from the one exponential.
//  2. Where the dispatcher puts a grid of 2 x CUs workgroups of the decode's shape (512 threads,
//     64 KB of LDS: two per compute unit): the key by which the de-phased grid of
//     scripts/ablations/loc_dephased_grid.patch takes its arrival tickets -- XCC id, and bits
//     15:8 of HW_ID -- must name each compute unit, i.e. be shared by exactly two workgroups.
//     Prints the histogram of workgroups per key, and how the two workgroups of a key differ
//     in blockIdx (measured: 256 keys of two workgroups, every pair 256 apart).
//   hipcc -O2 --offload-arch=gfx950 scripts/diag/fixed_cost_probe.hip -o build_diag/fixed_cost_probe
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));               \
            return 1;                                                             \
        }                                                                         \
    } while (0)

__global__ void exp_same(unsigned long long *bad, unsigned long long *nan) {
    const uint32_t base = (blockIdx.x * blockDim.x + threadIdx.x) << 8;  // 2^24 threads x 256 values
    unsigned nb = 0, nn = 0;
    for (uint32_t i = 0; i < 256u; ++i) {
        const float x = __uint_as_float(base + i);
        if (x != x) {
            ++nn;
            continue;
        }
        const float a = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(x, -23.0f, 23.0f));
        const float E = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(x, -126.0f, 126.0f));
        const float b = __builtin_amdgcn_fmed3f(E, 0x1p-23f, 0x1p23f);
        nb += __float_as_uint(a) != __float_as_uint(b);
    }
    if (nb) atomicAdd(bad, (unsigned long long)nb);
    if (nn) atomicAdd(nan, (unsigned long long)nn);
}

__global__ __launch_bounds__(512) void place(uint32_t *out, int spin) {
    extern __shared__ float lds[];
    float x = (float)threadIdx.x;
    for (int i = 0; i < spin; ++i) x = x * 1.0000001f + 1.0f;  // stay resident while the grid fills
    lds[threadIdx.x] = x;
    if (threadIdx.x == 0) {
        uint32_t xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        out[2 * blockIdx.x] = xcc;
        out[2 * blockIdx.x + 1] = hw;
    }
}

int main() {
    unsigned long long *d_cnt, h_cnt[2] = {0, 0};
    CHECK(hipMalloc(&d_cnt, sizeof(h_cnt)));
    CHECK(hipMemset(d_cnt, 0, sizeof(h_cnt)));
    hipLaunchKernelGGL(exp_same, dim3(1u << 16), dim3(256), 0, 0, d_cnt, d_cnt + 1);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost));
    printf("exp identity: %llu mismatches over %llu non-NaN floats\n", h_cnt[0], (1ull << 32) - h_cnt[1]);

    int cus = 0;
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const int grid = 2 * cus;
    uint32_t *d_out;
    std::vector<uint32_t> h(2 * (size_t)grid);
    CHECK(hipMalloc(&d_out, h.size() * 4));
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(place), hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    hipLaunchKernelGGL(place, dim3(grid), dim3(512), 65536, 0, d_out, 200000);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(h.data(), d_out, h.size() * 4, hipMemcpyDeviceToHost));
    std::map<uint32_t, std::vector<int>> by_key;
    for (int b = 0; b < grid; ++b) by_key[(h[2 * b] << 8) | ((h[2 * b + 1] >> 8) & 0xFFu)].push_back(b);
    std::map<size_t, int> hist;
    std::map<int, int> diff;
    int same_parity = 0, pairs = 0;
    for (auto &kv : by_key) {
        ++hist[kv.second.size()];
        if (kv.second.size() == 2) {
            ++pairs;
            ++diff[kv.second[1] - kv.second[0]];
            same_parity += (kv.second[0] & 1) == (kv.second[1] & 1);
        }
    }
    printf("placement: %d CUs, grid %d, %zu keys;", cus, grid, by_key.size());
    for (auto &kv : hist) printf(" %d keys with %zu workgroups;", kv.second, kv.first);
    printf(" %d of %d pairs have blockIdx of one parity\n", same_parity, pairs);
    printf("blockIdx difference within a pair (difference: pairs):");
    for (auto &kv : diff) printf(" %d: %d", kv.first, kv.second);
    printf("\nfirst workgroups (blockIdx xcc hw_id):");
    for (int b = 0; b < 12 && b < grid; ++b) printf(" %d %u %08x;", b, h[2 * b], h[2 * b + 1]);
    printf("\n");
    return h_cnt[0] == 0 ? 0 : 2;
}
