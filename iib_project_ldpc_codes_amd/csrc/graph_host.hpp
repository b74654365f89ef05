// Graph preparation (graph_host.cpp): edge lists or CSR -> validated host graph -> the kernels'
// layouts.  Host-only and pure: no HIP call, no environment variable (the C ABI reads the
// environment into LayoutOptions, capi.cpp), so it links and runs without a device
// (tests/host_layouts_main.cpp).
#pragma once
#include "errors.hpp"

namespace ldpc {

struct HostGraph {
    int n = 0, m = 0, k = 0, dv = 0, dc = 0;
    std::vector<int32_t> cvar, cptr, vptr, vchk, vslot;
    bool consistent = false;
    int max_vdeg = 0, max_cdeg = 0;
};

// Both validate their arguments and return LDPC_OK or LDPC_EINVAL (set_error says why).
int host_graph_from_lists(const int32_t *v2c, const int32_t *c2v, int n, int k, int dv, int dc, HostGraph &h);
int host_graph_from_csr(const int32_t *cptr, const int32_t *cvar, const int32_t *vptr, const int32_t *vslot, int n,
                        int m, HostGraph &h);

void build_lane_layout(const HostGraph &h, int T, int VPT, std::vector<int32_t> &lane_var,
                       std::vector<int32_t> &lane_slot);
bool build_irr_layout(const HostGraph &h, int &VPT, int &KC, int &DC, int &S, int &P, std::vector<int32_t> &lane,
                      std::vector<int32_t> &cdeg);

// Layer schedule of the layered (row-serial) decoder: the checks split into layers 0 .. L-1, no two
// checks of a layer sharing a variable -- a deterministic colouring of the check-conflict graph
// by kLayerRule.  layer[c]: the layer of check c; ptr [L+1] / chk [m]: the checks in (layer,
// falling degree, id) order; tab / var: the kernel's tables (ldpc_internal.hpp, kLayerTab).
// false (and L = 0) unless the graph is consistent, has 1 <= check degree <= 32 everywhere and no
// check holds a variable twice.
extern const char *const kLayerRule;
struct LayerSchedule {
    int L = 0, max_layer = 0;
    std::vector<int32_t> layer, ptr, chk, tab, var;
};
bool build_layer_schedule(const HostGraph &h, LayerSchedule &S);

// The soft-decoder layouts of a graph, built on the host: the arrays device_graph uploads.
struct HostLayouts {
    std::vector<int32_t> lane_var, lane_slot, irr_lane, irr_cdeg;
    LocLayout loc;
    LocChainLayout chain;
    LayerSchedule lay;
};

struct LayoutOptions {
    bool loc_layout = true;  // build the local-edge layout (off: tests run the other kernels on the same graphs)
    int loc_T = 0;           // threads of the local-edge layout, 0 = the shipped choice
    bool loc_chain = true;   // build the chained layout beside it (off: tests and A/B runs of the plain one)
};

// Fills g and, with layouts, the kernels' layouts (L and the lane_* / irr_* / loc_* scalars of g).
// layouts = false: the BEC decoders' graph only (the drop-in message_passing).
void host_layouts(const HostGraph &h, GraphShape &g, HostLayouts &L, bool layouts = true,
                  const LayoutOptions &opt = LayoutOptions());

}  // namespace ldpc
