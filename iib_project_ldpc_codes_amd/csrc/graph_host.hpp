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
// The tables of a schedule whose S.layer is given (every layer in use, no two checks of a layer
// sharing a variable): S.L, S.max_layer, ptr, chk, tab, var.  build_layer_schedule ends in it.
void layer_tables(const HostGraph &h, LayerSchedule &S);

// A quasi-cyclic code: H is an mb x nb array of Z x Z circulant permutations or zero blocks,
// base[r][c] = -1 for a zero block, otherwise the shift 0 <= s < Z.  Expansion (the header's,
// ldpc_graph_create_qc): check r Z + i holds variable c Z + (i + s_rc) mod Z for every non-zero
// cell of block row r, in ascending block-column order (the slot order); a variable's checks are
// in ascending check id.  The block rows are the layers (kQcLayerRule).
// row [mb][kQcRow]: bp_qc_q_kernel's table (ldpc_internal.hpp).
extern const char *const kQcLayerRule;
struct QcCode {
    int Z = 0, mb = 0, nb = 0;
    std::vector<int32_t> row;
};
// Validates (LDPC_EINVAL: Z < 1, a shift outside [0, Z), an all-zero block row or column, a
// block-row degree above 32) and expands.
int host_graph_from_qc(int mb, int nb, int Z, const int32_t *base, HostGraph &h, QcCode &qc);

// The soft-decoder layouts of a graph, built on the host: the arrays device_graph uploads.
struct HostLayouts {
    std::vector<int32_t> lane_var, lane_slot, irr_lane, irr_cdeg;
    LocLayout loc;
    LocChainLayout chain;
    LayerSchedule lay;
    std::vector<int32_t> qc_row;  // QcCode::row of a quasi-cyclic graph that runs bp_qc_q_kernel
};

struct LayoutOptions {
    bool loc_layout = true;  // build the local-edge layout (off: tests run the other kernels on the same graphs)
    int loc_T = 0;           // threads of the local-edge layout, 0 = the shipped choice
    bool loc_chain = true;   // build the chained layout beside it (off: tests and A/B runs of the plain one)
    bool loc_tq = true;      // ... decoded by the instantiation of its width where there is one (off: the generic one)
    const QcCode *qc = nullptr;  // the graph is this quasi-cyclic code's expansion: its block rows are the layers
    bool qc_kernel = true;       // ... and it runs bp_qc_q_kernel (off: the table kernels on the block-row schedule)
};

// Fills g and, with layouts, the kernels' layouts (L and the lane_* / irr_* / loc_* scalars of g).
// layouts = false: the BEC decoders' graph only (the drop-in message_passing).
void host_layouts(const HostGraph &h, GraphShape &g, HostLayouts &L, bool layouts = true,
                  const LayoutOptions &opt = LayoutOptions());

}  // namespace ldpc
