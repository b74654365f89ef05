// Error reporting of the host files (capi.cpp, graph_host.cpp, graph_device.cpp, mc_run.cpp): an
// entry point returns an LDPC_* code (ldpc_mi355x.h) and leaves the reason in set_error.
#pragma once
#include "ldpc_internal.hpp"
#include "ldpc_mi355x.h"

#define LDPC_HIP(expr)                                                                            \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            ldpc::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                   \
            return LDPC_EHIP;                                                                     \
        }                                                                                         \
    } while (0)
#define LDPC_TRY(call)            \
    do {                          \
        const int _rc = (call);   \
        if (_rc) return _rc;      \
    } while (0)
#define LDPC_REQUIRE(cond, msg)          \
    do {                                 \
        if (!(cond)) {                   \
            ldpc::set_error(msg);        \
            return LDPC_EINVAL;          \
        }                                \
    } while (0)
