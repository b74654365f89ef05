// The device side of a prepared graph (graph_device.cpp): upload, destroy, and the drop-in
// message_passing's cache of the last graph with its in-place refill.
#pragma once
#include "graph_host.hpp"

namespace ldpc {

int require_device();  // LDPC_OK, or LDPC_ENODEV: there is no CPU compute path

// h's arrays and its layouts (layouts = false: the BEC arrays only) on the current device.
int device_graph(const HostGraph &h, ldpc_graph **out, bool layouts, const LayoutOptions &opt);
void destroy_device_graph(ldpc_graph *g);

// Drop-in state (message_passing, one word per call): the reference re-sends the same
// fixed-code lists on every call (parallel_simulator.py:360, fresh numpy copies each time), so
// the last lists are kept on the host and compared exactly (memcmp: no hash to collide); their
// BEC-only device graph, a stream, and pinned staging for the word / error curve in one
// transfer each way.  The caller serialises all use (capi.cpp's g_mu).
struct DropInCache {
    int n = -1, k = -1, dv = -1, dc = -1, dev = -1;
    std::vector<int32_t> v2c, c2v;  // the lists of the cached graph (empty: none the graph is known to match)
    ldpc_graph *g = nullptr;
    hipStream_t s = nullptr;
    unsigned char *pin = nullptr, *dbuf = nullptr;  // [word u8 | errors i32 | its i32]
    size_t bytes = 0;

    // Makes g the graph of these lists on `device` (the current one): the cached graph when the
    // lists are the last call's, refilled in place when only their contents changed, else rebuilt.
    int lookup_or_build(const int32_t *v2c_new, const int32_t *c2v_new, int n_, int k_, int dv_, int dc_, int device);
    // The stream, and pin / dbuf of at least `need` bytes.
    int staging(size_t need);
};

}  // namespace ldpc
