// Backward of the diagonal feature warp (warp.hip: warp_feature_kernel) with respect to the features:
// g_out [B,V,D,H,W] -> g_src [B,V,D,H,W].
//
// The forward is linear in src -- out[b,v,k,y,x] = bilinear(src[b,v,k], pos_k(b,v,y,x)), zeros padding, align_corners=False --
// so nothing of it is saved:
//     g_src[b,v,k,t] = sum over the samples (y,x) of image (b,v,k) of g_out[b,v,k,y,x] w_tap(t),   over their in-bounds taps.
// Positions, taps and weights are the forward's bit for bit: both kernels run the per-sample chain of warp_sample.hpp.  The taps
// follow ATen's grid_sampler_2d backward: an in-bounds tap receives g w even when w == 0 (an infinite g then leaves a NaN there),
// an out-of-bounds tap receives nothing, a non-finite position has no tap (mask 0).
//
// One body (warp_bwd_body) for a contribution q = g w, handed to one of the three sinks of fixed_accum.hpp:
//   FloatAtomics  atomicAdd(float*) into g_src, zeroed on the stream first (one global_atomic_add_f32, no compare-and-swap loop).
//                 The grid is the forward's: the lanes of a wave are 64 consecutive pixels of one plane, whose taps fall on
//                 contiguous texel segments for the model's poses.  16 bytes of adds per sample: 67 MB at B = 4, V + 1 = 2, D = 64,
//                 64 x 128.  The last bits depend on the order of arrival.
//   MaxOfAbs, IntegerSum  the two passes of the deterministic path (max_exponent_pass, max_exponent_scatter): S_b from the exact
//                 maximum of |q| of the item and N = H W -- a sample puts at most one of its taps on any texel of its own
//                 (b,v,k) image.  An item whose maximum is 0 is exactly 0; an item with a non-finite contribution is NaN in every
//                 element; every other item is untouched by it -- as the other _det entries (scatter_det.hip).
// Workspace of the deterministic path: a 256-byte-rounded header of 4 bytes per item, then one int64 per element of g_src.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "fixed_accum.hpp"
#include "kernels.hpp"
#include "warp_sample.hpp"

namespace pdepth {

namespace {

using namespace fixed;
using namespace warp_sample;

constexpr int MAX_PLANES = 512;   // as the sweep's backward

// the most contributions a texel can receive (the kernel's and the convert pass's exponents both come from it)
__host__ __device__ inline long long max_contributions(const SweepArgs& a) { return (long long)a.H * a.W; }

// One thread: the pixel blockIdx.x * 256 + threadIdx.x of view v = blockIdx.y / nchunk of item blockIdx.z, planes chunk,
// chunk + nchunk, ...  `at` is an element of the contiguous [B,V,D,H,W] gradient; only in-bounds taps are formed, so every index
// handed to the sink lies inside the sample's own (b,v,k) image.
template <class Sink>
__device__ __forceinline__ void warp_bwd_body(const SweepArgs& a, int nchunk, const float* __restrict__ gout, Sink& sink) {
    const int HW = a.H * a.W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const bool live = pix < HW;
    const int pc = live ? pix : HW - 1;   // dead lanes shadow the last pixel and add nothing
    const int v = blockIdx.y / nchunk, chunk = blockIdx.y - v * nchunk;
    const int b = blockIdx.z;
    PixelChain c;
    make_pixel_chain(a, b, v, pc, c);
    const long long image0 = (((long long)b * a.V + v) * a.D) * HW;
    const float* g = gout + image0 + pc;
    for (int k = chunk; k < a.D; k += nchunk) {
        const Footprint f = plane_footprint(a, c, k);
        const unsigned m = live ? f.mask : 0u;
        if (!m) continue;
        const float gv = g[(size_t)k * HW];
        const long long at = image0 + (long long)k * HW + (f.y0 * a.W + f.x0);   // (the nw tap: may lie outside, then unused)
        if (m & 1u) sink.add(at, gv * f.nw);
        if (m & 2u) sink.add(at + 1, gv * f.ne);
        if (m & 4u) sink.add(at + a.W, gv * f.sw);
        if (m & 8u) sink.add(at + a.W + 1, gv * f.se);
    }
}

__global__ __launch_bounds__(256) void warp_bwd_kernel(SweepArgs a, int nchunk, const float* __restrict__ gout, float* __restrict__ gsrc) {
    FloatAtomics sink{gsrc};
    warp_bwd_body(a, nchunk, gout, sink);
}

// PASS 0: maximum of |q| per item; PASS 1: the integer scatter
template <int PASS>
__global__ __launch_bounds__(256) void warp_bwd_det_kernel(SweepArgs a, int nchunk, const float* __restrict__ gout, uint32_t* __restrict__ hdr,
                                                           unsigned long long* __restrict__ acc) {
    max_exponent_pass<PASS>(hdr + blockIdx.z, acc, max_contributions(a), [&](auto& sink) { warp_bwd_body(a, nchunk, gout, sink); });
}

size_t per_item(const SweepArgs& a) { return (size_t)a.V * a.D * a.H * a.W; }

}  // namespace

hipError_t launch_warp_feature_backward(const SweepArgs& a, const float* grad_out, float* grad_src, hipStream_t stream) {
    hipError_t e = launch_zero(grad_src, (size_t)a.B * per_item(a) * sizeof(float), stream);
    if (e != hipSuccess) return e;
    const int nchunk = plane_chunks(a);
    hipLaunchKernelGGL(warp_bwd_kernel, grid(a, nchunk), dim3(256), 0, stream, a, nchunk, grad_out, grad_src);
    return hipGetLastError();
}

size_t warp_feature_backward_det_workspace_bytes(int B, int V, int D, int H, int W) {
    return det_workspace_bytes(B, MaxExponent::WORDS, (size_t)V * D * H * W);
}

hipError_t launch_warp_feature_backward_det(const SweepArgs& a, const float* grad_out, float* grad_src, void* workspace, hipStream_t stream) {
    const int nchunk = plane_chunks(a);
    auto launch = [&](auto pass, uint32_t* hdr, unsigned long long* acc) {
        hipLaunchKernelGGL(warp_bwd_det_kernel<decltype(pass)::value>, grid(a, nchunk), dim3(256), 0, stream, a, nchunk, grad_out, hdr, acc);
    };
    return max_exponent_scatter(workspace, a.B, per_item(a), max_contributions(a), grad_src, stream, launch);
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h), beside the kernels like the entries of scatter_det.hip ---------------------------------------------
using namespace pdepth;
using namespace pdepth::capi;

namespace {

// what the two backward entries ask of their arguments alike
int check_warp_backward(const char* who, const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* d_candi, const float* grad_out,
                        const float* grad_src) {
    if (int rc = check_desc(desc, cam, who)) return rc;
    if (!d_candi || !grad_out || !grad_src) return fail(PDEPTH_E_ARG, "%s: null input pointer", who);
    if (desc->C != desc->D) return fail(PDEPTH_E_ARG, "%s: needs C == D (got C=%d D=%d)", who, desc->C, desc->D);
    if (desc->D > MAX_PLANES) return fail(PDEPTH_E_ARG, "%s: D=%d exceeds the %d planes one launch supports", who, desc->D, MAX_PLANES);
    if (int rc = check_launch_limits(who, desc->B, desc->H, desc->W)) return rc;
    const long long chw = (long long)desc->D * desc->H * desc->W;
    if (desc->src_vstride != chw || desc->src_bstride != chw * desc->V)
        return fail(PDEPTH_E_ARG, "%s: bad strides (grad_src must be contiguous [B,V,D,H,W])", who);
    if (grad_out == grad_src) return fail(PDEPTH_E_ARG, "%s: grad_src may not alias grad_out", who);
    return PDEPTH_OK;
}

}  // namespace

extern "C" {

int pdepth_warp_feature_backward_f32(const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* d_candi, const float* grad_out,
                                     float* grad_src, void* stream) {
    const char* who = "pdepth_warp_feature_backward_f32";
    if (int rc = check_warp_backward(who, desc, cam, d_candi, grad_out, grad_src)) return rc;
    const SweepArgs a = make_args(desc, cam, nullptr, nullptr, d_candi);
    return launched(launch_warp_feature_backward(a, grad_out, grad_src, (hipStream_t)stream), who);
}

size_t pdepth_warp_feature_backward_det_workspace_bytes(const pdepth_sweep_desc* desc) {
    if (!desc || !dims_positive(desc) || desc->C != desc->D || desc->D > MAX_PLANES || (long long)desc->H * desc->W > (1ll << 30)) return 0;
    return warp_feature_backward_det_workspace_bytes(desc->B, desc->V, desc->D, desc->H, desc->W);
}

int pdepth_warp_feature_backward_det_f32(const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* d_candi, const float* grad_out,
                                         float* grad_src, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pdepth_warp_feature_backward_det_f32";
    if (int rc = check_warp_backward(who, desc, cam, d_candi, grad_out, grad_src)) return rc;
    const size_t need = warp_feature_backward_det_workspace_bytes(desc->B, desc->V, desc->D, desc->H, desc->W);
    if (int rc = check_workspace(who, workspace, workspace_bytes, need, "; query pdepth_warp_feature_backward_det_workspace_bytes()")) return rc;
    const SweepArgs a = make_args(desc, cam, nullptr, nullptr, d_candi);
    return launched(launch_warp_feature_backward_det(a, grad_out, grad_src, workspace, (hipStream_t)stream), who);
}

}  // extern "C"
