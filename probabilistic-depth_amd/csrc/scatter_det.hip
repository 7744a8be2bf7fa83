// The two scattered gradients of the training loss as order-independent sums (fixed_accum.hpp): g_src_depth of the depth stereo
// consistency term (loss_terms.hip: loss_dsc_bwd_kernel) and grad_img of inverse_warp (inverse_warp.hip: inverse_warp_bwd_kernel, both
// sampling modes).  The same bits from call to call, and an item's result does not depend on its neighbours in the batch.
//
// Both are one-thread-per-pixel kernels, and each has one scatter body -- dsc_scatter (loss_terms_math.hpp), scatter_sample
// (inverse_warp_math.hpp) -- which the atomic kernels call with FloatAtomics and the kernels here with the sinks of the two passes
// (fixed_accum.hpp: max_exponent_pass on the device, max_exponent_scatter on the host): the contributions are the atomic path's
// bit for bit because they are formed by the same code.
//   pass 0  the exact maximum of |q| over the contributions of an item (atomicMax over the bit patterns of |q|: order-independent,
//           a NaN or an infinity wins it) -> S_b = det_scale_exponent(max, N), N = 4 H W (pixels x taps: max_contributions);
//   pass 1  the same contributions, quantised with S_b and added to the int64 accumulator (global_atomic_add_x2);
//   convert accumulator -> fp32.  An item whose maximum is 0 is 0; an item with a non-finite contribution is NaN in every element
//           (an integer cannot hold a NaN; the atomic path confines it to the texels it reaches), every other item is untouched.
// The gradients that are written per owner -- g_tgt_depth, grad_point -- are those of the existing kernels, called with a null
// scatter pointer: the same bits as the atomic path's.
//
// Workspace: a 256-byte-rounded header of 4 bytes per item, then one int64 per element of the scattered gradient.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "fixed_accum.hpp"
#include "inverse_warp_math.hpp"
#include "kernels.hpp"
#include "loss_terms_math.hpp"

namespace pdepth {

namespace {

using namespace fixed;

// the header word of an item is the maximum of |q| over its contributions (fixed_accum.hpp: MaxExponent, put_max)
size_t workspace_bytes(int B, size_t per_item) { return det_workspace_bytes(B, MaxExponent::WORDS, per_item); }

// the most contributions one element of either gradient can receive: every pixel of the map, four taps each (the kernels' and
// the convert pass's exponents both come from it)
__host__ __device__ inline long long max_contributions(int H, int W) { return 4ll * H * W; }

// PASS 0: maximum of |v|; PASS 1: scatter.  grid (blocks of 256 pixels, B)
template <int PASS>
__global__ __launch_bounds__(256) void dsc_det_kernel(DscArgs g, const float* __restrict__ count, const float* __restrict__ g_value,
                                                      uint32_t* __restrict__ hdr, unsigned long long* __restrict__ acc) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = g.H * g.W;
    const int b = blockIdx.y;
    DscGrad d{0.0f, 0.0f, -1};   // a lane past the map: no tap
    if (pix < HW) d = dsc_pixel_grad(g, count, g_value, b, pix);
    max_exponent_pass<PASS>(hdr + b, acc, max_contributions(g.H, g.W), [&](auto& sink) { dsc_scatter(d, (long long)b * HW, sink); });
}

// grad_img of inverse_warp_bwd_kernel<MODE>: q = g (nearest) / g w_t (bilinear) at the in-bounds taps
template <int MODE, int PASS>
__global__ __launch_bounds__(256) void inverse_warp_det_kernel(const float* __restrict__ depth, const float* __restrict__ Kinv,
                                                               const float* __restrict__ proj, const float* __restrict__ go, int C, int H,
                                                               int W, uint32_t* __restrict__ hdr, unsigned long long* __restrict__ acc) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    const int b = blockIdx.y;
    const bool live = pix < HW;
    const int pc = live ? pix : HW - 1;   // dead lanes shadow the last pixel and add nothing
    const int y = pc / W, x = pc - y * W;
    const WarpSample q = warp_sample(Kinv + b * 9, proj + b * 12, x, y, depth[(size_t)b * HW + pc], H, W);
    const long long image0 = (long long)b * C * HW;
    max_exponent_pass<PASS>(hdr + b, acc, max_contributions(H, W),
                            [&](auto& sink) { scatter_sample<MODE>(q, live, go + image0 + pc, image0, C, H, W, sink); });
}

}  // namespace

}  // namespace pdepth

// ---- C ABI (include/pdepth.h), beside the kernels like the entries of loss_terms.hip ------------------------------------------------
using namespace pdepth;
using namespace pdepth::capi;

extern "C" {

size_t pdepth_loss_dsc_backward_det_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return (B > 0 && H > 0 && W > 0 && (long long)H * W <= (1ll << 24)) ? workspace_bytes(B, (size_t)H * W) : 0;
}

size_t pdepth_inverse_warp_backward_det_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    return (B > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W <= (1ll << 30)) ? workspace_bytes(B, (size_t)C * H * W) : 0;
}

int pdepth_loss_dsc_backward_det_f32(const float* src_depth, const float* tgt_depth, const float* src_mask, const float* Kinv,
                                     const float* proj, const float* pose_row, int32_t pose_batched, const float* intr, const float* count,
                                     const float* g_value, int32_t B, int32_t H, int32_t W, float* g_src_depth, float* g_tgt_depth,
                                     void* workspace, size_t workspace_bytes_given, void* stream) {
    const char* who = "pdepth_loss_dsc_backward_det_f32";
    if (!src_depth || !tgt_depth || !src_mask || !Kinv || !proj || !pose_row || !intr || !count || !g_value)
        return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!g_src_depth && !g_tgt_depth) return fail(PDEPTH_E_ARG, "%s: no gradient requested", who);
    if (int rc = check_map(who, B, H, W, 2)) return rc;
    const size_t per_item = (size_t)H * W;
    if (g_src_depth) {
        if (int rc = check_workspace(who, workspace, workspace_bytes_given, workspace_bytes(B, per_item),
                                     "; query pdepth_loss_dsc_backward_det_workspace_bytes()"))
            return rc;
    }
    if (g_tgt_depth) {   // written per owner: the existing kernel, nothing scattered
        if (int rc = pdepth_loss_dsc_backward_f32(src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, pose_batched, intr, count, g_value, B,
                                                  H, W, nullptr, g_tgt_depth, stream))
            return rc;
    }
    if (!g_src_depth) return PDEPTH_OK;
    hipStream_t s = (hipStream_t)stream;
    const DscArgs a{src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr, pose_batched ? 4 : 0, H, W};
    const dim3 grid((unsigned)((per_item + 255) / 256), B);
    auto launch = [&](auto pass, uint32_t* hdr, unsigned long long* acc) {
        hipLaunchKernelGGL(dsc_det_kernel<decltype(pass)::value>, grid, dim3(256), 0, s, a, count, g_value, hdr, acc);
    };
    return launched(max_exponent_scatter(workspace, B, per_item, max_contributions(H, W), g_src_depth, s, launch), who);
}

int pdepth_inverse_warp_backward_det_f32(const float* img, const float* depth, const float* Kinv, const float* proj, const float* grad_out,
                                         int32_t B, int32_t C, int32_t H, int32_t W, int32_t mode, float* grad_img, float* grad_point,
                                         void* workspace, size_t workspace_bytes_given, void* stream) {
    const char* who = "pdepth_inverse_warp_backward_det_f32";
    if (!img || !depth || !Kinv || !proj || !grad_out || (!grad_img && !grad_point)) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (B <= 0 || C <= 0 || H <= 1 || W <= 1) return fail(PDEPTH_E_ARG, "%s: bad dimension", who);
    if (mode != PDEPTH_SAMPLE_BILINEAR && mode != PDEPTH_SAMPLE_NEAREST) return fail(PDEPTH_E_ARG, "%s: unknown mode %d", who, mode);
    if (int rc = check_launch_limits(who, B, H, W)) return rc;
    const size_t per_item = (size_t)C * H * W;
    if (grad_img) {
        if (int rc = check_workspace(who, workspace, workspace_bytes_given, workspace_bytes(B, per_item),
                                     "; query pdepth_inverse_warp_backward_det_workspace_bytes()"))
            return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    if (grad_point) {   // written per owner: the existing kernel, nothing scattered
        if (int rc = launched(launch_inverse_warp_backward(img, depth, Kinv, proj, grad_out, B, C, H, W, mode, nullptr, grad_point, s), who))
            return rc;
    }
    if (!grad_img) return PDEPTH_OK;
    const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), B);
    auto launch = [&](auto pass, uint32_t* hdr, unsigned long long* acc) {
        constexpr int PASS = decltype(pass)::value;
        auto kern = mode == PDEPTH_SAMPLE_BILINEAR ? inverse_warp_det_kernel<0, PASS> : inverse_warp_det_kernel<1, PASS>;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, depth, Kinv, proj, grad_out, C, H, W, hdr, acc);
    };
    return launched(max_exponent_scatter(workspace, B, per_item, max_contributions(H, W), grad_img, s, launch), who);
}

}  // extern "C"
