// Device graphs: see graph_device.hpp.
#include "graph_device.hpp"

#include <cstring>
#include <utility>


namespace ldpc {
namespace {

// The device arrays of a graph, each with the host vector it is filled from: the one list that
// upload, the drop-in's refill and destroy walk (f(device pointer, host vector) -> hipError_t,
// stopping at the first failure).  A new layout array is added here and nowhere else.
template <typename F>
hipError_t for_graph_arrays(ldpc_graph &g, const HostGraph &h, const HostLayouts &L, F f) {
    static const std::vector<int32_t> none;
    const std::pair<int32_t **, const std::vector<int32_t> *> arrays[] = {
        {&g.cvar, &h.cvar},           {&g.cptr, &h.cptr},
        {&g.vptr, &h.vptr},           {&g.vchk, &h.vchk},
        {&g.vslot, h.consistent ? &h.vslot : &none},  // defined only for consistent lists
        {&g.lane_var, &L.lane_var},   {&g.lane_slot, &L.lane_slot},
        {&g.loc_var, &L.loc.var},     {&g.loc_pos, &L.loc.pos},
        {&g.loc_info, &L.loc.info},   {&g.irr_lane, &L.irr_lane},
        {&g.irr_cdeg, &L.irr_cdeg},
        {&g.chn_var, &L.chain.var},   {&g.chn_pos, &L.chain.pos},
        {&g.chn_info, &L.chain.info},
        {&g.lay_tab, &L.lay.tab},     {&g.lay_var, &L.lay.var},
        {&g.lay_cbase, &L.lay.ptr},   {&g.qc_row, &L.qc_row},
    };
    for (const auto &a : arrays) {
        const hipError_t e = f(*a.first, *a.second);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t upload(int32_t *&dst, const std::vector<int32_t> &src) {
    dst = nullptr;
    if (src.empty()) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&dst), src.size() * 4);
    if (e != hipSuccess) return e;
    return hipMemcpy(dst, src.data(), src.size() * 4, hipMemcpyHostToDevice);
}

// New contents in arrays of the same sizes (an empty host vector has no device array)
hipError_t refill(int32_t *&dst, const std::vector<int32_t> &src) {
    return src.empty() ? hipSuccess : hipMemcpy(dst, src.data(), src.size() * 4, hipMemcpyHostToDevice);
}

}  // namespace

int require_device() {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("libldpc_mi355x: no HIP device visible (this library has no CPU path; run on an MI355X)");
        return LDPC_ENODEV;
    }
    return LDPC_OK;
}

int device_graph(const HostGraph &h, ldpc_graph **out, bool layouts, const LayoutOptions &opt) {
    LDPC_TRY(require_device());
    ldpc_graph *g = new ldpc_graph();
    HostLayouts L;
    host_layouts(h, *g, L, layouts, opt);
    (void)hipGetDevice(&g->device);
    const hipError_t e = for_graph_arrays(*g, h, L, upload);
    if (e != hipSuccess) {
        set_error(std::string("graph upload: ") + hipGetErrorString(e));
        destroy_device_graph(g);
        return LDPC_EHIP;
    }
    *out = g;
    return LDPC_OK;
}

void destroy_device_graph(ldpc_graph *g) {
    if (!g) return;
    (void)for_graph_arrays(*g, HostGraph(), HostLayouts(), [](int32_t *&d, const std::vector<int32_t> &) {
        (void)hipFree(d);
        return hipSuccess;
    });
    delete g;
}

int DropInCache::lookup_or_build(const int32_t *v2c_new, const int32_t *c2v_new, int n_, int k_, int dv_, int dc_,
                                 int device) {
    const size_t Ev = (size_t)n_ * dv_, Ec = (size_t)(n_ - k_) * dc_;
    const bool same_shape = g && n == n_ && k == k_ && dv == dv_ && dc == dc_ && dev == device;
    if (same_shape && v2c.size() == Ev && c2v.size() == Ec && !memcmp(v2c.data(), v2c_new, Ev * 4) &&
        !memcmp(c2v.data(), c2v_new, Ec * 4))
        return LDPC_OK;
    HostGraph hg;
    LDPC_TRY(host_graph_from_lists(v2c_new, c2v_new, n_, k_, dv_, dc_, hg));
    if (same_shape && g->consistent == hg.consistent && g->vchk_len == (int)hg.vchk.size()) {
        // another graph of the same shape (an ensemble run: a new code per trial): new contents
        // in the same device arrays.  No lists are cached while the copies run: were one to
        // fail, the half-new graph must match no later call's lists.
        v2c.clear();
        c2v.clear();
        LDPC_HIP(for_graph_arrays(*g, hg, HostLayouts(), refill));
        g->max_vdeg = hg.max_vdeg;
        g->max_cdeg = hg.max_cdeg;
    } else {
        destroy_device_graph(g);
        g = nullptr;
        if (s && dev != device) {  // the stream and buffers belong to the old device
            (void)hipStreamDestroy(s);
            (void)hipHostFree(pin);
            (void)hipFree(dbuf);
            s = nullptr;
            pin = dbuf = nullptr;
            bytes = 0;
        }
        LDPC_TRY(device_graph(hg, &g, false, LayoutOptions()));
        n = n_; k = k_; dv = dv_; dc = dc_; dev = device;
    }
    v2c.assign(v2c_new, v2c_new + Ev);
    c2v.assign(c2v_new, c2v_new + Ec);
    return LDPC_OK;
}

int DropInCache::staging(size_t need) {
    if (!s) LDPC_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (need <= bytes) return LDPC_OK;
    (void)hipHostFree(pin);
    (void)hipFree(dbuf);
    pin = dbuf = nullptr;
    bytes = 0;
    LDPC_HIP(hipHostMalloc(reinterpret_cast<void **>(&pin), need, hipHostMallocDefault));
    LDPC_HIP(hipMalloc(reinterpret_cast<void **>(&dbuf), need));
    bytes = need;
    return LDPC_OK;
}

}  // namespace ldpc
