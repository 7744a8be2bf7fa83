// DPV Bayesian fusion, forward: kernels, launcher and C entry (pdepth_dpv_fuse_f32).
//
// Upsample mode (models/models.py:666-672 with utils/img_utils.py:31-47, :360-375): build the Gaussian soft label of a sparse depth
// map over the depth candidates, blend it with the uniform DPV by the validity mask, multiply it into the network's DPV,
// renormalise, clamp, take the log -- one kernel, one read of the log-DPV, two writes, instead of ~12 passes.
// Its backward with respect to the log-DPV is csrc/dpv_fuse_bwd.hip (same lane layout, same helpers).
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "dpv_fuse_math.hpp"

namespace pdepth {

// Single pass: lane = pixel, the D planes of the column live in registers between the three sweeps over k (Gaussian
// and its sum; fused product and its sum; normalise + write), so the log-DPV is read once and each output written
// once: 4*HW*(D*(1+outputs)+2) bytes.  DREG = planes held in registers (64 or 128); deeper volumes take the
// re-reading kernel below.
// exp / log / divide: fuse_exp / fuse_log / fuse_div / fuse_rcp of dpv_fuse_math.hpp, shared with the backward.
template <int DREG>
__global__ __launch_bounds__(256) void dpv_fuse_reg_kernel(const float* __restrict__ logp,
                                                           const float* __restrict__ dmaps,
                                                           const float* __restrict__ masks,
                                                           const float* __restrict__ dc, int D, int HW, float var,
                                                           float eps, float* __restrict__ fused,
                                                           float* __restrict__ logfused) {
    __shared__ float s_dc[DREG];
    for (int k = threadIdx.x; k < DREG; k += 256) s_dc[k] = k < D ? dc[k] : 0.0f;
    __syncthreads();
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const float dmap = dmaps[(size_t)b * HW + pix];
    const float mask = masks[(size_t)b * HW + pix];
    const float inv_mask = 1.0f - mask;
    const float sigma = sqrtf(var);
    const float two_var = 2.0f * (sigma * sigma);  // 2 * torch.pow(sig, 2)
    const float r_two_var = fuse_rcp(two_var);
    const float uni = 1.0f / (float)D;
    const float* lp = logp + (size_t)b * D * HW + pix;
    float v[DREG], x[DREG];
#pragma unroll
    for (int k = 0; k < DREG; ++k) x[k] = k < D ? __builtin_nontemporal_load(lp + (size_t)k * HW) : 0.0f;
    float sumg = 0.0f;
#pragma unroll
    for (int k = 0; k < DREG; ++k) {
        const float a = fabsf(s_dc[k] - dmap);
        v[k] = fuse_exp(fuse_div(-(a * a), two_var, r_two_var));
        if (k < D) sumg = sumg + v[k];
    }
    float sumf = 0.0f;
    const float r_sumg = fuse_rcp(sumg);
#pragma unroll
    for (int k = 0; k < DREG; ++k) {
        float t = fuse_div(v[k], sumg, r_sumg);
        if (t != t) t = -1.0f;                       // zero_invalid (img_utils.py:45)
        const float m = t * mask + uni * inv_mask;   // img_utils.py:371
        v[k] = fuse_exp(x[k] + fuse_log(fminf(fmaxf(m, eps), 1.0f)));
        if (k < D) sumf = sumf + v[k];
    }
    const float r_sumf = fuse_rcp(sumf);
    float* of = fused ? fused + (size_t)b * D * HW + pix : nullptr;
    float* ol = logfused ? logfused + (size_t)b * D * HW + pix : nullptr;
#pragma unroll
    for (int k = 0; k < DREG; ++k) {
        if (k < D) {
            const float f = fminf(fmaxf(fuse_div(v[k], sumf, r_sumf), eps), 1.0f);
            if (of) __builtin_nontemporal_store(f, of + (size_t)k * HW);
            if (ol) __builtin_nontemporal_store(fuse_log(f), ol + (size_t)k * HW);
        }
    }
}

// Any D: the column is re-read (from L2) in the second and third sweep.
__global__ __launch_bounds__(256) void dpv_fuse_kernel(const float* __restrict__ logp,
                                                       const float* __restrict__ dmaps,
                                                       const float* __restrict__ masks,
                                                       const float* __restrict__ dc, int D, int HW, float var,
                                                       float eps, float* __restrict__ fused,
                                                       float* __restrict__ logfused) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const float dmap = dmaps[(size_t)b * HW + pix];
    const float mask = masks[(size_t)b * HW + pix];
    const float inv_mask = 1.0f - mask;
    const float sigma = sqrtf(var);
    const float two_var = 2.0f * (sigma * sigma);  // 2 * torch.pow(sig, 2)
    const float uni = 1.0f / (float)D;
    const float* lp = logp + (size_t)b * D * HW + pix;
    float sumg = 0.0f;
    for (int k = 0; k < D; ++k) {
        const float a = fabsf(dc[k] - dmap);
        sumg = sumg + expf(-(a * a) / two_var);
    }
    auto tofuse = [&](int k) {
        const float a = fabsf(dc[k] - dmap);
        float t = expf(-(a * a) / two_var) / sumg;
        if (t != t) t = -1.0f;                       // zero_invalid (img_utils.py:45)
        const float m = t * mask + uni * inv_mask;   // img_utils.py:371
        // fmaxf / fminf return the other operand for a NaN: a NaN m (or q below) becomes eps, where torch.clamp keeps the NaN.
        // A NaN, an all -inf or an overflowing column of logp comes out as eps on every plane.
        return fminf(fmaxf(m, eps), 1.0f);
    };
    float sumf = 0.0f;
    for (int k = 0; k < D; ++k) sumf = sumf + expf(lp[(size_t)k * HW] + logf(tofuse(k)));
    float* of = fused ? fused + (size_t)b * D * HW + pix : nullptr;
    float* ol = logfused ? logfused + (size_t)b * D * HW + pix : nullptr;
    for (int k = 0; k < D; ++k) {
        float f = expf(lp[(size_t)k * HW] + logf(tofuse(k))) / sumf;
        f = fminf(fmaxf(f, eps), 1.0f);
        if (of) of[(size_t)k * HW] = f;
        if (ol) ol[(size_t)k * HW] = logf(f);
    }
}

static hipError_t launch_dpv_fuse(const float* logp, const float* dmaps, const float* masks, const float* d_candi,
                                  int B, int D, int H, int W, float var, float eps, float* fused, float* logfused,
                                  hipStream_t stream) {
    dim3 grid((H * W + 255) / 256, B);
    if (D <= 64)
        hipLaunchKernelGGL(dpv_fuse_reg_kernel<64>, grid, dim3(256), 0, stream, logp, dmaps, masks, d_candi, D, H * W, var, eps, fused, logfused);
    else if (D <= 128)
        hipLaunchKernelGGL(dpv_fuse_reg_kernel<128>, grid, dim3(256), 0, stream, logp, dmaps, masks, d_candi, D, H * W, var, eps, fused, logfused);
    else
        hipLaunchKernelGGL(dpv_fuse_kernel, grid, dim3(256), 0, stream, logp, dmaps, masks, d_candi, D, H * W, var, eps, fused, logfused);
    return hipGetLastError();
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h) -------------------------------------------------------------------------------------------------------
using namespace pdepth::capi;

extern "C" int pdepth_dpv_fuse_f32(const float* logp, const float* dmaps, const float* masks, const float* d_candi,
                                   int32_t B, int32_t D, int32_t H, int32_t W, float var, float eps, float* fused,
                                   float* logfused, void* stream) {
    if (!logp || !dmaps || !masks || !d_candi) return fail(PDEPTH_E_ARG, "pdepth_dpv_fuse_f32: null input");
    if (!fused && !logfused) return fail(PDEPTH_E_ARG, "pdepth_dpv_fuse_f32: no output requested");
    if (int rc = check_dims("pdepth_dpv_fuse_f32", B, D, H, W)) return rc;
    if (int rc = check_launch_limits("pdepth_dpv_fuse_f32", B, H, W)) return rc;   // (B is grid.y, like in the backward)
    if (!(var > 0.0f)) return fail(PDEPTH_E_ARG, "pdepth_dpv_fuse_f32: var must be positive");
    return launched(pdepth::launch_dpv_fuse(logp, dmaps, masks, d_candi, B, D, H, W, var, eps, fused, logfused,
                                            (hipStream_t)stream), "pdepth_dpv_fuse_f32");
}
