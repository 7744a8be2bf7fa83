// What the C entries (include/pdepth.h) of capi.hip, dpv_fuse.hip, dpv_moments.hip, correlation.hip, inverse_warp.hip, loss.hip, loss_terms.hip, metrics.hip, lidar_depth.hip, dpv_fuse_bwd.hip,
// sweep_bwd_det.hip, scatter_det.hip, warp_bwd.hip, ssim.hip, photo.hip, ternary.hip, occlusion.hip, flow_warp.hip, loss_smooth1.hip and flow_metrics.hip check and report alike.
// Inline, and in need of nothing but pdepth::api_error (capi.o): an object that includes this refers to no other object, so a
// library linked from a subset of the objects (tests/test_sweep_prefetch.py) still links.  (cost_volume.hip and flow_photo.hip
// also include this; they alone need a second object, flow_warp.o, whose backward the first launches and whose check of sizes
// and pad both call: flow_warp_launch.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>

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

// B, H, W of a map walked one thread per pixel: positive, at least `least` rows and columns, H W <= 2^24 (a pixel count is exact
// in fp32), B within the grid's y
inline int check_map(const char* who, int32_t B, int32_t H, int32_t W, int least) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(PDEPTH_E_ARG, "%s: non-positive dimension", who);
    if (H < least || W < least) return fail(PDEPTH_E_ARG, "%s: H and W must be at least %d", who, least);
    if ((long long)H * W > (1ll << 24) || B > 65535) return fail(PDEPTH_E_ARG, "%s: H*W must be at most 2^24 and B at most 65535", who);
    return PDEPTH_OK;
}

// the half-width of a window or patch (`noun`: the word the message uses) of (2 md + 1)^2: md in 1..3, and H and W hold one
inline int check_window(const char* who, const char* noun, int32_t H, int32_t W, int32_t md) {
    if (md < 1 || md > 3) return fail(PDEPTH_E_ARG, "%s: md=%d: the %s is (2 md + 1)^2 with md = 1, 2 or 3", who, md, noun);
    if (H < 2 * md + 1 || W < 2 * md + 1)
        return fail(PDEPTH_E_ARG, "%s: H=%d, W=%d: md=%d needs H and W of at least %d", who, H, W, md, 2 * md + 1);
    return PDEPTH_OK;
}

// md (one that check_window passes) as a compile-time constant: f(std::integral_constant<int, 1 | 2 | 3>)
template <typename F>
inline void for_md(int md, F&& f) {
    if (md == 1) f(std::integral_constant<int, 1>{});
    else if (md == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 3>{});
}

// ---- the sweep descriptor (the entries of capi.hip and sweep_bwd_det.hip) ----
// every dimension positive of a descriptor
inline bool dims_positive(const pdepth_sweep_desc* d) { return d->B > 0 && d->V > 0 && d->C > 0 && d->D > 0 && d->H > 0 && d->W > 0; }
inline int check_desc_dims(const char* who, const pdepth_sweep_desc* d) {
    if (dims_positive(d)) return PDEPTH_OK;
    return fail(PDEPTH_E_ARG, "%s: non-positive dimension B=%d V=%d C=%d D=%d H=%d W=%d", who, d->B, d->V, d->C, d->D, d->H, d->W);
}

inline int check_desc(const pdepth_sweep_desc* d, const pdepth_camera* cam, const char* who) {
    if (!d || !cam) return fail(PDEPTH_E_ARG, "%s: null descriptor", who);
    if (int rc = check_desc_dims(who, d)) return rc;
    if ((long long)d->H * d->W > (1ll << 30))
        return fail(PDEPTH_E_ARG, "%s: H*W too large", who);
    if (!cam->K || !cam->R || !cam->t || !cam->rays || !cam->cxcy)
        return fail(PDEPTH_E_ARG, "%s: null camera pointer", who);
    if (d->blas_mode != PDEPTH_BLAS_FMA && d->blas_mode != PDEPTH_BLAS_SEPARATE)
        return fail(PDEPTH_E_ARG, "%s: unknown blas_mode %d", who, d->blas_mode);
    const long long chw = (long long)d->C * d->H * d->W;
    if (d->src_vstride < chw || d->src_bstride < 0 || d->ref_bstride < 0)
        return fail(PDEPTH_E_ARG, "%s: bad strides", who);
    return PDEPTH_OK;
}

// the one place a SweepArgs is filled from a descriptor (cam == nullptr: the entries that launch no sampling kernel)
inline SweepArgs make_args(const pdepth_sweep_desc* d, const pdepth_camera* cam = nullptr, const float* ref = nullptr,
                           const float* src = nullptr, const float* d_candi = nullptr) {
    SweepArgs a{};
    a.ref = ref; a.src = src; a.packed_src = nullptr;
    if (cam) { a.K = cam->K; a.R = cam->R; a.t = cam->t; a.rays = cam->rays; a.cxcy = cam->cxcy; }
    a.d_candi = d_candi;
    a.B = d->B; a.V = d->V; a.C = d->C; a.D = d->D; a.H = d->H; a.W = d->W;
    a.metric = d->metric; a.sigma = d->sigma; a.blas_mode = d->blas_mode;
    a.fast_div = d->algo != PDEPTH_ALGO_DIRECT;
    a.ref_bstride = d->ref_bstride; a.src_bstride = d->src_bstride; a.src_vstride = d->src_vstride;
    return a;
}


// what pdepth_sweep_backward_f32 and pdepth_sweep_backward_det_f32 ask of their arguments alike
inline int check_sweep_backward(const char* who, const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* ref, const float* src,
                                const float* d_candi, const float* grad_cost, const float* grad_ref, const float* grad_src) {
    if (int rc = check_desc(desc, cam, who)) return rc;
    if (!ref || !src || !d_candi || !grad_cost) return fail(PDEPTH_E_ARG, "%s: null input pointer", who);
    if (!grad_ref && !grad_src) return fail(PDEPTH_E_ARG, "%s: no output requested", who);
    if (desc->metric != PDEPTH_METRIC_L2 && desc->metric != PDEPTH_METRIC_L1)
        return fail(PDEPTH_E_ARG, "%s: undefined metric for feature distance (%d)", who, desc->metric);
    if (!(desc->sigma > 0.0f) && !(desc->sigma < 0.0f)) return fail(PDEPTH_E_ARG, "%s: sigma must be non-zero", who);
    if (desc->D > 512) return fail(PDEPTH_E_ARG, "%s: D=%d exceeds the 512 planes one launch supports", who, desc->D);
    if ((long long)desc->C * desc->H * desc->W >= (1ll << 31) || desc->B > 65535)
        return fail(PDEPTH_E_ARG, "%s: C*H*W must be below 2^31 and B at most 65535", who);
    if ((const void*)grad_ref == (const void*)grad_src || (const float*)grad_ref == ref || (const float*)grad_src == src ||
        (const float*)grad_ref == grad_cost || (const float*)grad_src == grad_cost)
        return fail(PDEPTH_E_ARG, "%s: the outputs may not alias each other or an input", who);
    return PDEPTH_OK;
}

}  // namespace capi
}  // namespace pdepth
