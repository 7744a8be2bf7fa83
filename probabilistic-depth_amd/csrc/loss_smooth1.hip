// First-order smoothness of a flow: smooth_grad_1st (losses/loss_blocks.py:210-220), the smoothness term of the unsupervised flow
// loss (losses/flow_loss.py:29-32).  flo [B,Cf,H,W], image [B,Ci,H,W], ONE value for the batch -- the means run over it:
//     wx = exp(-alpha mean_c |image[..., x+1] - image[..., x]|),   value = mean(wx |dx flo|) / 4 + mean(wy |dy flo|) / 4
// over [B,Cf,H,W-1] and [B,Cf,H-1,W].  One thread per pixel: the pair's weight once (the channel sum in channel order), then the
// flow's channels.  The sum is the loss terms' (loss_terms_sum.hpp): per-workgroup partial sums, added in a fixed order in double by
// one workgroup -- the partial sums of all items read as those of one.  The same bits from call to call.
// Backward, with respect to flo only (image is data): a per-owner gather, every flow value collecting its left / right and up /
// down differences with sign(0) = 0, as abs has in torch.  No atomics.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "loss_terms_math.hpp"
#include "loss_terms_sum.hpp"

namespace pdepth {

namespace {

// exp(-alpha mean_c |image - image'|) of the pair (pix, pix + step) of an item's image [Ci][HW]
__device__ __forceinline__ float smooth1_weight(const float* __restrict__ im, int Ci, int HW, int pix, int step, float alpha) {
    float a = 0.0f;
    for (int c = 0; c < Ci; ++c) a += fabsf(im[(size_t)c * HW + pix + step] - im[(size_t)c * HW + pix]);
    return expf(-(a / (float)Ci) * alpha);
}

// sums of w |d flo| along x and along y; grid (blocks of 256 pixels, B)
__global__ __launch_bounds__(256) void loss_smooth1_kernel(const float* __restrict__ flo, const float* __restrict__ image, int Cf,
                                                           int Ci, int H, int W, float alpha, float* __restrict__ part) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    float sx = 0.0f, sy = 0.0f;
    if (pix < HW) {
        const int b = blockIdx.y;
        const int y = pix / W, x = pix - y * W;
        const float* f = flo + (size_t)b * Cf * HW;
        const float* im = image + (size_t)b * Ci * HW;
        if (x < W - 1) {
            const float w = smooth1_weight(im, Ci, HW, pix, 1, alpha);
            for (int c = 0; c < Cf; ++c) sx += w * fabsf(f[(size_t)c * HW + pix + 1] - f[(size_t)c * HW + pix]);
        }
        if (y < H - 1) {
            const float w = smooth1_weight(im, Ci, HW, pix, W, alpha);
            for (int c = 0; c < Cf; ++c) sy += w * fabsf(f[(size_t)c * HW + pix + W] - f[(size_t)c * HW + pix]);
        }
    }
    block_partial({sx, sy}, part);
}

// gx = g / (4 Nx), gy = g / (4 Ny): the weights of the four pairs a pixel takes part in, then the flow's channels
__global__ __launch_bounds__(256) void loss_smooth1_bwd_kernel(const float* __restrict__ flo, const float* __restrict__ image,
                                                               const float* __restrict__ g_value, int Cf, int Ci, int H, int W, float alpha,
                                                               float nx4, float ny4, float* __restrict__ g_flo) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const int y = pix / W, x = pix - y * W;
    const float* im = image + (size_t)b * Ci * HW;
    const float gx = g_value[0] / nx4, gy = g_value[0] / ny4;
    const float wr = x < W - 1 ? gx * smooth1_weight(im, Ci, HW, pix, 1, alpha) : 0.0f;
    const float wl = x > 0 ? gx * smooth1_weight(im, Ci, HW, pix - 1, 1, alpha) : 0.0f;
    const float wd = y < H - 1 ? gy * smooth1_weight(im, Ci, HW, pix, W, alpha) : 0.0f;
    const float wu = y > 0 ? gy * smooth1_weight(im, Ci, HW, pix - W, W, alpha) : 0.0f;
    for (int c = 0; c < Cf; ++c) {
        const float* f = flo + ((size_t)b * Cf + c) * HW;
        const float v = f[pix];
        float out = 0.0f;
        if (x > 0) out += wl * sign0(v - f[pix - 1]);
        if (x < W - 1) out -= wr * sign0(f[pix + 1] - v);
        if (y > 0) out += wu * sign0(v - f[pix - W]);
        if (y < H - 1) out -= wd * sign0(f[pix + W] - v);
        g_flo[((size_t)b * Cf + c) * HW + pix] = out;
    }
}

// what the two entries ask of their sizes alike (the pair counts 4 Nx, 4 Ny enter as fp32: one rounding above 2^24)
int check_smooth1(const char* who, int32_t B, int32_t Cf, int32_t Ci, int32_t H, int32_t W, float alpha) {
    if (Cf <= 0 || Ci <= 0) return capi::fail(PDEPTH_E_ARG, "%s: non-positive dimension", who);
    if (int rc = capi::check_map(who, B, H, W, 2)) return rc;
    if ((long long)B * n_blocks(H, W) > (1ll << 30)) return capi::fail(PDEPTH_E_ARG, "%s: too many workgroups", who);
    if (alpha != alpha) return capi::fail(PDEPTH_E_ARG, "%s: alpha is NaN", who);
    return PDEPTH_OK;
}

inline float pairs4(int B, int Cf, int rows, int cols) { return 4.0f * (float)((long long)B * Cf * rows * cols); }

}  // namespace

}  // namespace pdepth

// ---- C ABI (include/pdepth.h), beside the kernels like the entries of loss_terms.hip ------------------------------------------------
using namespace pdepth;
using namespace pdepth::capi;

extern "C" {

int pdepth_loss_smooth1_f32(const float* flo, const float* image, int32_t B, int32_t Cf, int32_t Ci, int32_t H, int32_t W, float alpha,
                            float* value, void* workspace, size_t workspace_bytes_given, void* stream) {
    const char* who = "pdepth_loss_smooth1_f32";
    if (!flo || !image) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!value) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_smooth1(who, B, Cf, Ci, H, W, alpha)) return rc;
    if (int rc = check_workspace(who, workspace, workspace_bytes_given, two_sums_workspace_bytes(B, H, W))) return rc;
    const int nblk = n_blocks(H, W);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(loss_smooth1_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, flo, image, Cf, Ci, H, W, alpha, part);
    // the partial sums of all items as those of one: [2][B][nblk] read as [2][1][B nblk]
    return launched(finish<false>(part, 1, B * nblk, pairs4(B, Cf, H, W - 1), pairs4(B, Cf, H - 1, W), value, nullptr, (hipStream_t)stream), who);
}

int pdepth_loss_smooth1_backward_f32(const float* flo, const float* image, const float* g_value, int32_t B, int32_t Cf, int32_t Ci,
                                     int32_t H, int32_t W, float alpha, float* g_flo, void* stream) {
    const char* who = "pdepth_loss_smooth1_backward_f32";
    if (!flo || !image || !g_value || !g_flo) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_smooth1(who, B, Cf, Ci, H, W, alpha)) return rc;
    hipLaunchKernelGGL(loss_smooth1_bwd_kernel, dim3(n_blocks(H, W), B), dim3(256), 0, (hipStream_t)stream, flo, image, g_value, Cf, Ci, H,
                       W, alpha, pairs4(B, Cf, H, W - 1), pairs4(B, Cf, H - 1, W), g_flo);
    return launched(hipGetLastError(), who);
}

}  // extern "C"
