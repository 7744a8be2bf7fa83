// Backward of the DPV reductions (dpv.hip) with respect to their volume input.
//
// dpv_reduce / dpv_reduce_ex: x = logits (+ addend) -> logp = log_softmax(x, dim=1) (models/models.py:560,637,694;
// packnet.py:394), prob = exp(logp) (models/models.py:697), depth = sum_k d_k prob_k (utils/img_utils.py:52-61).  Given the
// saved logp and any of the incoming gradients g_logp, g_prob, g_depth:
//     G_k = g_logp_k + p_k (g_prob_k + g_depth d_k),    g_x_k = G_k - p_k sum_j G_j,    p = exp(logp)
// dpv_expect: depth = sum_k d_k (bv_log ? exp(dpv_k) : dpv_k)  ->  g_dpv_k = g_depth d_k (bv_log ? exp(dpv_k) : 1).
// One thread per pixel, the planes in a loop (the lanes of a wave read consecutive pixels of a plane row); no atomics: the
// results are reproducible bit for bit.
#include <hip/hip_runtime.h>

#include "dpv_reduce_body.hpp"
#include "kernels.hpp"

namespace pdepth {

namespace {

__global__ __launch_bounds__(256) void dpv_reduce_bwd_kernel(const float* __restrict__ logp, const float* __restrict__ dc, int D, int HW,
                                                             const float* __restrict__ g_logp, const float* __restrict__ g_prob,
                                                             const float* __restrict__ g_depth, float* __restrict__ g_x) {
    dpv_reduce_bwd_pixel(logp, dc, D, HW, g_logp, g_prob, g_depth, g_x);   // (dpv_reduce_body.hpp, shared with dpv_half.hip)
}

__global__ __launch_bounds__(256) void dpv_expect_bwd_kernel(const float* __restrict__ dpv, const float* __restrict__ dc, int D, int HW,
                                                             int bv_log, const float* __restrict__ g_depth, float* __restrict__ g_dpv) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= HW) return;
    const size_t b = blockIdx.y;
    const size_t base = b * D * HW + pix;
    const float gd = g_depth[b * HW + pix];
    for (int k = 0; k < D; ++k) {
        const size_t i = base + (size_t)k * HW;
        const float gk = gd * dc[k];
        g_dpv[i] = bv_log ? gk * expf(dpv[i]) : gk;
    }
}

}  // namespace

hipError_t launch_dpv_reduce_backward(const float* logp, const float* d_candi, int B, int D, int H, int W, const float* g_logp,
                                      const float* g_prob, const float* g_depth, float* g_logits, hipStream_t stream) {
    const int HW = H * W;
    hipLaunchKernelGGL(dpv_reduce_bwd_kernel, dim3((HW + 255) / 256, B), dim3(256), 0, stream, logp, d_candi, D, HW, g_logp, g_prob,
                       g_depth, g_logits);
    return hipGetLastError();
}

hipError_t launch_dpv_expect_backward(const float* dpv, const float* d_candi, int B, int D, int H, int W, int bv_log,
                                      const float* g_depth, float* g_dpv, hipStream_t stream) {
    const int HW = H * W;
    hipLaunchKernelGGL(dpv_expect_bwd_kernel, dim3((HW + 255) / 256, B), dim3(256), 0, stream, dpv, d_candi, D, HW, bv_log, g_depth,
                       g_dpv);
    return hipGetLastError();
}

}  // namespace pdepth
