// What the C entries (include/pdepth.h) of capi.hip, loss.hip, loss_terms.hip, metrics.hip, lidar_depth.hip and dpv_fuse_bwd.hip check and report alike.
// Inline, and in need of nothing but pdepth::api_error (capi.o): an object that includes this refers to no other object, so a
// library linked from a subset of the objects (tests/test_sweep_prefetch.py) still links.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/pdepth.h"
#include "kernels.hpp"

namespace pdepth {
namespace capi {

// sets the message pdepth_last_error() returns on this thread, returns code
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char* fmt, ...) {
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    return api_error(code, msg);
}

inline int launched(hipError_t e, const char* who) {
    if (e != hipSuccess) return fail(PDEPTH_E_LAUNCH, "%s: %s", who, hipGetErrorString(e));
    return PDEPTH_OK;
}

// every dimension positive, of the entries that take B, D (or C), H, W as plain arguments
inline int check_dims(const char* who, int32_t B, int32_t D, int32_t H, int32_t W) {
    if (B > 0 && D > 0 && H > 0 && W > 0) return PDEPTH_OK;
    return fail(PDEPTH_E_ARG, "%s: non-positive dimension", who);
}

// what a launch of one workgroup per 256 pixels (grid x) and item (grid y) can take
inline int check_launch_limits(const char* who, int32_t B, int32_t H, int32_t W) {
    if ((long long)H * W <= (1ll << 30) && B <= 65535) return PDEPTH_OK;
    return fail(PDEPTH_E_ARG, "%s: H*W must be at most 2^30 and B at most 65535", who);
}

// a workspace: present, large enough, 256-byte aligned (hint: appended to the message of the first two)
inline int check_workspace(const char* who, const void* workspace, size_t bytes, size_t need, const char* hint = "") {
    if (!workspace || bytes < need)
        return fail(PDEPTH_E_WORKSPACE, "%s: needs %zu bytes of workspace (got %zu)%s", who, need, bytes, hint);
    if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0)
        return fail(PDEPTH_E_WORKSPACE, "%s: workspace must be 256-byte aligned", who);
    return PDEPTH_OK;
}

}  // namespace capi
}  // namespace pdepth
