// Occlusion masks for the stereo consistency terms: the range map of a forward splat and its threshold (utils/warp_utils.py:
// get_corresponding_map :25-79, get_occu_mask_backward :102-108 of the reference).
//
//   r[b, y, x] = sum over the source pixels p of the bilinear weight with which p's position lands on (x, y);
//   visible    = (min(max(r, 0), 1) < th) ? 0 : 1        (1 - the reference's occluded mask)
// Only in-bounds taps count, a non-finite position adds nothing.  Two entry forms over one scatter body (splat):
//   positions  coords [B,2,H,W], un-normalised (x, y): the footprint of sample_at (inverse_warp_math.hpp), the products of WarpSample;
//   depth      depth [B,H,W] (+ src_mask), Kinv, proj: the position warp_sample computes for the consistency term of the opposite
//              direction, W / (W - 1) convention included -- the mask describes the warp the loss performs.
// The sum is always the integer sum of fixed_accum.hpp: a float atomicAdd would let a mass within an ulp of th flip a mask bit with
// the order of arrival.  Every weight lies in [0, 1] and a destination receives at most one tap per source pixel, so the exponent
// S = det_scale_exponent(1, H W) is known on the host: clear the accumulator, one scatter pass, one convert pass that writes the
// range map, the mask or both.  One source pixel per lane, lanes along W; grid (blocks of 256 pixels of an item, B).
//
// Workspace: one int64 per pixel, [B][H W], rounded up to 256 bytes.
#include <hip/hip_runtime.h>

#include <cmath>

#include "capi_util.hpp"
#include "fixed_accum.hpp"
#include "inverse_warp_math.hpp"

namespace pdepth {

namespace {

using namespace fixed;

size_t workspace_bytes(int B, size_t per_item) { return det_workspace_bytes(B, FixedExponent::WORDS, per_item); }

// the exponent of both the scatter and the convert pass: weights <= 1, at most H W contributions to a destination
inline int range_exponent(int H, int W) { return det_scale_exponent(1.0f, (int64_t)H * W); }

// one source pixel's weights to the in-bounds taps of its position; item0: the first element of the item's map
template <class Sink>
__device__ __forceinline__ void splat(const WarpSample& q, bool live, long long item0, int W, Sink& sink) {
    const TapMask t = tap_mask(q);
    const TapMask m{live && t.nw, live && t.ne, live && t.sw, live && t.se};
    if (m.any()) scatter_taps(q, m, item0 + (q.y0 * W + q.x0), W, 1.0f, sink);
}

__global__ __launch_bounds__(256) void range_coords_kernel(const float* __restrict__ coords, int H, int W, IntegerSum sink) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const float* c = coords + (size_t)b * 2 * HW + pix;
    splat(sample_at(c[0], c[HW], H, W), true, (long long)b * HW, W, sink);
}

__global__ __launch_bounds__(256) void range_depth_kernel(const float* __restrict__ depth, const float* __restrict__ src_mask,
                                                          const float* __restrict__ Kinv, const float* __restrict__ proj, int H, int W,
                                                          IntegerSum sink) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const size_t at = (size_t)b * HW + pix;
    const int y = pix / W, x = pix - y * W;
    const bool live = !src_mask || src_mask[at] != 0.0f;
    splat(warp_sample(Kinv + b * 9, proj + b * 12, x, y, depth[at], H, W), live, (long long)b * HW, W, sink);
}

// accumulator -> range map and / or visibility mask (either pointer may be null)
__global__ __launch_bounds__(256) void range_convert_kernel(const long long* __restrict__ acc, int S, float th, float* __restrict__ range,
                                                            float* __restrict__ visible, int HW) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const size_t at = (size_t)blockIdx.y * HW + pix;
    const float r = det_to_float(acc[at], S);
    if (range) range[at] = r;
    if (visible) visible[at] = fminf(fmaxf(r, 0.0f), 1.0f) < th ? 0.0f : 1.0f;
}

// what both entries ask of their outputs, sizes and workspace alike, before any launch
int check_range(const char* who, int32_t B, int32_t H, int32_t W, int least, float th, const float* range, const float* visible,
                const void* workspace, size_t workspace_bytes_given, const char* hint) {
    if (!range && !visible) return capi::fail(PDEPTH_E_ARG, "%s: no output requested", who);
    if (int rc = capi::check_map(who, B, H, W, least)) return rc;
    if (std::isnan(th)) return capi::fail(PDEPTH_E_ARG, "%s: th is NaN", who);
    return capi::check_workspace(who, workspace, workspace_bytes_given, workspace_bytes(B, (size_t)H * W), hint);
}

// clear, scatter (launch(sink)), convert
template <class Launch>
int run_range(const char* who, int B, int H, int W, float th, float* range, float* visible, void* workspace, hipStream_t s, Launch launch) {
    const int S = range_exponent(H, W);
    const size_t per_item = (size_t)H * W;
    if (int rc = capi::launched(fixed_exponent_scatter(workspace, B, per_item, S, s, launch), who)) return rc;
    const dim3 grid((unsigned)((per_item + 255) / 256), B);
    hipLaunchKernelGGL(range_convert_kernel, grid, dim3(256), 0, s,
                       reinterpret_cast<const long long*>(det_accumulator(workspace, B, FixedExponent::WORDS)), S, th, range, visible, H * W);
    return capi::launched(hipGetLastError(), who);
}

}  // namespace

}  // namespace pdepth

// ---- C ABI (include/pdepth.h), beside the kernels like the entries of scatter_det.hip ----------------------------------------------
using namespace pdepth;
using namespace pdepth::capi;

extern "C" {

size_t pdepth_range_map_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return (B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= (1ll << 24)) ? workspace_bytes(B, (size_t)H * W) : 0;
}

int pdepth_range_map_f32(const float* coords, int32_t B, int32_t H, int32_t W, float th, float* range, float* visible, void* workspace,
                         size_t workspace_bytes_given, void* stream) {
    const char* who = "pdepth_range_map_f32";
    if (!coords) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_range(who, B, H, W, 1, th, range, visible, workspace, workspace_bytes_given, "; query pdepth_range_map_workspace_bytes()"))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), B);
    return run_range(who, B, H, W, th, range, visible, workspace, s,
                     [&](fixed::IntegerSum sink) { hipLaunchKernelGGL(range_coords_kernel, grid, dim3(256), 0, s, coords, H, W, sink); });
}

int pdepth_depth_range_map_f32(const float* depth, const float* src_mask, const float* Kinv, const float* proj, int32_t B, int32_t H,
                               int32_t W, float th, float* range, float* visible, void* workspace, size_t workspace_bytes_given,
                               void* stream) {
    const char* who = "pdepth_depth_range_map_f32";
    if (!depth || !Kinv || !proj) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_range(who, B, H, W, 2, th, range, visible, workspace, workspace_bytes_given, "; query pdepth_range_map_workspace_bytes()"))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), B);
    return run_range(who, B, H, W, th, range, visible, workspace, s, [&](fixed::IntegerSum sink) {
        hipLaunchKernelGGL(range_depth_kernel, grid, dim3(256), 0, s, depth, src_mask, Kinv, proj, H, W, sink);
    });
}

}  // extern "C"
