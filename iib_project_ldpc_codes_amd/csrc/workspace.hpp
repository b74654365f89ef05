// Per-(device, stream) device workspaces of the C ABI: grow-only buffers the entry points stage
// into and the launchers take their scratch from.
#pragma once
#include <map>
#include <mutex>
#include <utility>

#include "ldpc_internal.hpp"

namespace ldpc {

// Grow-only device buffer.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (p && bytes <= cap) return hipSuccess;  // (a first request for 0 bytes allocates too: p is never null after success)
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    // The buffer as `count` Ts, grown when needed; nullptr (and the reason in set_error) only when
    // the allocation fails.
    template <typename T>
    T *get(size_t count) {
        const hipError_t e = ensure(count * sizeof(T));
        if (e != hipSuccess) set_error(std::string("workspace allocation: ") + hipGetErrorString(e));
        return e == hipSuccess ? static_cast<T *>(p) : nullptr;
    }
};

// Lock order: the C ABI's g_mu (capi.cpp) before Workspace::mu; the device-pointer Monte-Carlo
// entries take only their workspace's lock, so launches on different devices / streams never
// serialise on g_mu.  ldpc_bp_decode_batch_dev takes both on every call and holds them across its
// (asynchronous) launch, on purpose: another thread growing the same workspace cannot free the
// scratch before the launch is queued; the cost is a brief serialisation of decode launches on g_mu.
struct Workspace {
    std::mutex mu;
    DevBuf trial, its, cutoff, scratch, words, llr, post, hard, errors, itsb, gchk, gvar, gatt, mlw, mlo, mlu, shape,
        sctl;  // sampler search control (sample_ctl_words)
};

inline Workspace &workspace(void *stream) {
    static std::mutex mu;  // the map (each workspace has its own lock)
    static std::map<std::pair<int, void *>, Workspace> ws;  // (device, stream)
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    return ws[std::make_pair(dev, stream)];  // std::map nodes never move
}

}  // namespace ldpc
