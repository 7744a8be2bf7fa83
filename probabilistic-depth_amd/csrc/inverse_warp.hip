// inverse_warp, forward and backward: kernels, launchers and C entries (pdepth_inverse_warp_f32, pdepth_inverse_warp_backward_f32).
//
// Replaces utils/inverse_warp.py:174-210: the depth-map driven warp used by the training losses (losses/loss_blocks.py:116
// bilinear, :151 'nearest').  pixel2cam (:26-40), cam2pixel (:43-69, Z clamped at 1e-3, coordinates normalised with (w-1), (h-1)),
// then F.grid_sample with its default align_corners=False, zeros padding.
// Forward: one kernel.  Backward: the same per-pixel chain re-evaluated, the image gradient scattered with atomics
// (like ATen's grid_sampler backward) and the gradient with respect to the projected point (X, Y, Z) written per
// pixel; the 3x3 / 3x4 algebra behind it (depth, pose, intrinsics) is a handful of small matmuls on the host side.
// The per-pixel chain (warp_sample, warp_valid, nearest_tap; tap_mask, load_texels, bilinear_value and its derivatives, point_grad;
// the scatter bodies scatter_taps / scatter_sample) is inverse_warp_math.hpp, shared with loss_terms.hip and scatter_det.hip.
// launch_inverse_warp_backward is declared in kernels.hpp: scatter_det.hip calls it for the gradient of the projected point.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "fixed_accum.hpp"
#include "geometry.hpp"
#include "inverse_warp_math.hpp"

namespace pdepth {

template <int MODE>   // 0 bilinear, 1 nearest
__global__ __launch_bounds__(256) void inverse_warp_kernel(const float* __restrict__ img,
                                                           const float* __restrict__ depth,
                                                           const float* __restrict__ Kinv,
                                                           const float* __restrict__ proj, int C, int H, int W,
                                                           float* __restrict__ out, unsigned char* __restrict__ valid) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const int y = pix / W, x = pix - y * W;
    const WarpSample q = warp_sample(Kinv + b * 9, proj + b * 12, x, y, depth[(size_t)b * HW + pix], H, W);
    if (valid) valid[(size_t)b * HW + pix] = warp_valid(q) ? 1 : 0;
    float* ob = out + (size_t)b * C * HW + pix;
    if (MODE == 1) {
        const int tap = nearest_tap(q, H, W);
        for (int c = 0; c < C; ++c) ob[(size_t)c * HW] = tap >= 0 ? img[((size_t)b * C + c) * HW + tap] : 0.0f;
        return;
    }
    const float* ib = img + (size_t)b * C * HW + (q.y0 * W + q.x0);
    const TapMask taps = tap_mask(q);
    for (int c = 0; c < C; ++c) ob[(size_t)c * HW] = bilinear_value(q, load_texels(ib + (size_t)c * HW, taps, W));
}

// grad_img [B,C,H,W] (zeroed by the launcher, atomics; may be NULL), grad_pc [B,3,H,W] = dL/d(X, Y, Z) of the
// projected point (zero in nearest mode, where the output does not depend on the position; may be NULL).
template <int MODE>
__global__ __launch_bounds__(256) void inverse_warp_bwd_kernel(const float* __restrict__ img,
                                                               const float* __restrict__ depth,
                                                               const float* __restrict__ Kinv,
                                                               const float* __restrict__ proj,
                                                               const float* __restrict__ go, int C, int H, int W,
                                                               float* __restrict__ grad_img, float* __restrict__ grad_pc) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const int y = pix / W, x = pix - y * W;
    const WarpSample q = warp_sample(Kinv + b * 9, proj + b * 12, x, y, depth[(size_t)b * HW + pix], H, W);
    const float* gb = go + (size_t)b * C * HW + pix;
    const long long image0 = (long long)b * C * HW;
    fixed::FloatAtomics sink{grad_img};
    float gix = 0.0f, giy = 0.0f;
    if (MODE == 1) {
        if (grad_img) scatter_sample<1>(q, true, gb, image0, C, H, W, sink);
    } else {
        // the channel loop of scatter_sample<0>, kept here: one load of g and of the texels feeds the position gradient and the scatter
        const long long base = image0 + (q.y0 * W + q.x0);
        const TapMask taps = tap_mask(q);
        for (int c = 0; c < C; ++c) {
            const float g = gb[(size_t)c * HW];
            const Texels v = load_texels(img + base + (long long)c * HW, taps, W);
            gix = __builtin_fmaf(g, bilinear_d_ix(q, v), gix);
            giy = __builtin_fmaf(g, bilinear_d_iy(q, v), giy);
            if (grad_img) scatter_taps(q, taps, base + (long long)c * HW, W, g, sink);
        }
    }
    if (grad_pc) {
        PointGrad gp{0.0f, 0.0f, 0.0f};
        if (MODE == 0 && q.finite) gp = point_grad(q, gix, giy, H, W);
        float* o = grad_pc + (size_t)b * 3 * HW + pix;
        o[0] = gp.X; o[HW] = gp.Y; o[2 * (size_t)HW] = gp.Z;
    }
}

static hipError_t launch_inverse_warp(const float* img, const float* depth, const float* Kinv, const float* proj, int B,
                                      int C, int H, int W, int mode, float* out, unsigned char* valid, hipStream_t stream) {
    dim3 grid((H * W + 255) / 256, B);
    if (mode == 0)
        hipLaunchKernelGGL(inverse_warp_kernel<0>, grid, dim3(256), 0, stream, img, depth, Kinv, proj, C, H, W, out, valid);
    else
        hipLaunchKernelGGL(inverse_warp_kernel<1>, grid, dim3(256), 0, stream, img, depth, Kinv, proj, C, H, W, out, valid);
    return hipGetLastError();
}

hipError_t launch_inverse_warp_backward(const float* img, const float* depth, const float* Kinv, const float* proj,
                                        const float* grad_out, int B, int C, int H, int W, int mode, float* grad_img,
                                        float* grad_pc, hipStream_t stream) {
    if (grad_img) {
        hipError_t e = launch_zero(grad_img, (size_t)B * C * H * W * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    dim3 grid((H * W + 255) / 256, B);
    if (mode == 0)
        hipLaunchKernelGGL(inverse_warp_bwd_kernel<0>, grid, dim3(256), 0, stream, img, depth, Kinv, proj, grad_out, C, H, W, grad_img, grad_pc);
    else
        hipLaunchKernelGGL(inverse_warp_bwd_kernel<1>, grid, dim3(256), 0, stream, img, depth, Kinv, proj, grad_out, C, H, W, grad_img, grad_pc);
    return hipGetLastError();
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h) -------------------------------------------------------------------------------------------------------
using namespace pdepth::capi;

extern "C" {

int pdepth_inverse_warp_f32(const float* img, const float* depth, const float* Kinv, const float* proj, int32_t B,
                            int32_t C, int32_t H, int32_t W, int32_t mode, float* out, uint8_t* valid, void* stream) {
    if (!img || !depth || !Kinv || !proj || !out) return fail(PDEPTH_E_ARG, "pdepth_inverse_warp_f32: null pointer");
    if (B <= 0 || C <= 0 || H <= 1 || W <= 1) return fail(PDEPTH_E_ARG, "pdepth_inverse_warp_f32: bad dimension");
    if (mode != PDEPTH_SAMPLE_BILINEAR && mode != PDEPTH_SAMPLE_NEAREST) return fail(PDEPTH_E_ARG, "pdepth_inverse_warp_f32: unknown mode %d", mode);
    return launched(pdepth::launch_inverse_warp(img, depth, Kinv, proj, B, C, H, W, mode, out, valid, (hipStream_t)stream),
                    "pdepth_inverse_warp_f32");
}

int pdepth_inverse_warp_backward_f32(const float* img, const float* depth, const float* Kinv, const float* proj,
                                     const float* grad_out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t mode,
                                     float* grad_img, float* grad_point, void* stream) {
    if (!img || !depth || !Kinv || !proj || !grad_out || (!grad_img && !grad_point))
        return fail(PDEPTH_E_ARG, "pdepth_inverse_warp_backward_f32: null pointer");
    if (B <= 0 || C <= 0 || H <= 1 || W <= 1) return fail(PDEPTH_E_ARG, "pdepth_inverse_warp_backward_f32: bad dimension");
    if (mode != PDEPTH_SAMPLE_BILINEAR && mode != PDEPTH_SAMPLE_NEAREST)
        return fail(PDEPTH_E_ARG, "pdepth_inverse_warp_backward_f32: unknown mode %d", mode);
    return launched(pdepth::launch_inverse_warp_backward(img, depth, Kinv, proj, grad_out, B, C, H, W, mode, grad_img,
                                                         grad_point, (hipStream_t)stream), "pdepth_inverse_warp_backward_f32");
}

}  // extern "C"
