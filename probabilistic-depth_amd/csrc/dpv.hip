// DPV reduction kernels: log-softmax over the depth axis + expectation, one pass over HBM.
//
// Replaces F.log_softmax(x, dim=1) (models/models.py:560,637,694,:351; packnet.py:394)
// followed by dpv_to_depthmap (utils/img_utils.py:52-61; called per item at
// trainer/default_trainer.py:229-233).  The reference makes 5 passes over the D x H x W
// volume (log_softmax read+write, exp, mul, sum); here the logits are read once, held in
// registers, and logp + depth are written once: 4*HW*(2D+1) bytes per item.
//
// The vec4 kernels use the wave layout of dpv_lanes.hpp: lane = (plane group, pixel quad), the column of a pixel spread over
// 4 lanes, per-pixel max / sum-exp / sum d*exp combined across the plane groups.
#include <hip/hip_runtime.h>

#include "dpv_lanes.hpp"
#include "dpv_reduce_body.hpp"
#include "kernels.hpp"

namespace pdepth {

// (DpvExtras and the bodies dpv_reduce_lanes / dpv_reduce_ex_pixel: dpv_reduce_body.hpp, shared with dpv_half.hip)

template <int RPL>
__global__ __launch_bounds__(256) void dpv_reduce_vec4_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ dc,
                                                              int D, int HW, float* logp,
                                                              float* __restrict__ depth) {
    dpv_reduce_lanes<RPL, false>(x, dc, D, HW, logp, depth, DpvExtras{});
}

// Any D / any HW: one pixel per thread, three sweeps over the column (re-reads hit L2).
__global__ __launch_bounds__(256) void dpv_reduce_scalar_kernel(const float* x,
                                                                const float* __restrict__ dc,
                                                                int D, int HW, float* logp,
                                                                float* __restrict__ depth) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const float* xb = x + (size_t)b * D * HW + pix;
    float m = -INFINITY;
    for (int k = 0; k < D; ++k) m = fmaxf(m, xb[(size_t)k * HW]);
    float s = 0.f;
    for (int k = 0; k < D; ++k) s += expf(xb[(size_t)k * HW] - m);
    const float ls = logf(s);
    float e = 0.f;
    float* lb = logp ? logp + (size_t)b * D * HW + pix : nullptr;
    for (int k = 0; k < D; ++k) {
        const float lp = (xb[(size_t)k * HW] - m) - ls;  // read before the aliasing store
        if (lb) lb[(size_t)k * HW] = lp;
        e += dc[k] * expf(lp);
    }
    if (depth) depth[(size_t)b * HW + pix] = e;
}

template <int RPL>
__global__ __launch_bounds__(256) void dpv_reduce_ex_vec4_kernel(const float* __restrict__ x, const float* __restrict__ dc,
                                                                 int D, int HW, float* logp, float* __restrict__ depth,
                                                                 DpvExtras ex) {
    dpv_reduce_lanes<RPL, true>(x, dc, D, HW, logp, depth, ex);
}

// any D / any H, W: one pixel per thread (re-reads hit L2)
__global__ __launch_bounds__(256) void dpv_reduce_ex_scalar_kernel(const float* x, const float* __restrict__ dc, int D,
                                                                   int HW, float* logp, float* __restrict__ depth,
                                                                   DpvExtras ex) {
    dpv_reduce_ex_pixel<false>(x, dc, D, HW, logp, depth, ex);
}

// Expectation in the wave layout: all loads of a lane issued up front (RPL 16-byte non-temporal loads in flight per lane).
// The load loop is written out: through load_planes, whose optional arguments are all constant here, the log-DPV instantiations
// were allocated and scheduled differently and ran 12 % (D = 64) and 48 % (D = 128) slower (profiles/r11_dpv_lanes/README.md).
template <bool BV_LOG, int RPL>
__global__ __launch_bounds__(256) void dpv_expect_vec4_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ dc, int D, int HW,
                                                              float* __restrict__ depth) {
    const QuadLane L = quad_lane(D, HW);
    float4 v[RPL];
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
        const int k = L.g + 4 * i;
        v[i] = (k < D && L.live) ? load_nt(x + L.off + (size_t)k * HW) : splat4(0.f);
    }
    float4 e = splat4(0.f);
    expect_planes<BV_LOG>(e, v, dc, L.g, 0, D);
    e = group_sum(e);
    if (L.live && L.g == 0) *reinterpret_cast<float4*>(depth + L.poff) = e;
}

template <bool BV_LOG, int VEC>
__global__ __launch_bounds__(256) void dpv_expect_kernel(const float* __restrict__ x,
                                                         const float* __restrict__ dc, int D,
                                                         int HW, float* __restrict__ depth) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = HW / VEC;
    if (i >= n) return;
    const int b = blockIdx.y;
    const float* xb = x + (size_t)b * D * HW + (size_t)i * VEC;
    float e[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) e[j] = 0.f;
    for (int k = 0; k < D; ++k) {
        const float dk = dc[k];
        float v[VEC];
        if (VEC == 4) {
            const float4 t = *reinterpret_cast<const float4*>(xb + (size_t)k * HW);
            v[0] = t.x; v[1 % VEC] = t.y; v[2 % VEC] = t.z; v[3 % VEC] = t.w;
        } else {
            v[0] = xb[(size_t)k * HW];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) e[j] += dk * (BV_LOG ? expf(v[j]) : v[j]);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) depth[(size_t)b * HW + (size_t)i * VEC + j] = e[j];
}

hipError_t launch_dpv_reduce(const float* logits, const float* d_candi, int B, int D, int H,
                             int W, float* logp, float* depth, hipStream_t stream) {
    const int HW = H * W;
    const bool vec = (HW % 4 == 0) && aligned16(logits) && (!logp || aligned16(logp)) &&
                     (!depth || aligned16(depth)) && D <= 128;
    const dim3 grid(n_blocks(H, W), B);
    if (vec) {
        for_planes_per_lane(D, [&](auto rpl) {
            hipLaunchKernelGGL(dpv_reduce_vec4_kernel<decltype(rpl)::value>, grid, dim3(256), 0, stream, logits, d_candi, D, HW, logp, depth);
        });
    } else {
        hipLaunchKernelGGL(dpv_reduce_scalar_kernel, grid, dim3(256), 0, stream, logits, d_candi, D, HW, logp, depth);
    }
    return hipGetLastError();
}

hipError_t launch_dpv_reduce_ex(const float* logits, const float* addend, const float* d_candi, int B, int D, int H, int W,
                                float* logp, float* prob, float* depth, float* variance, float* quarter, hipStream_t stream) {
    const int HW = H * W;
    DpvExtras ex{addend, prob, variance, quarter, W};
    const bool vec = (W % 4 == 0) && aligned16(logits) && (!addend || aligned16(addend)) && (!logp || aligned16(logp)) &&
                     (!prob || aligned16(prob)) && (!depth || aligned16(depth)) && (!variance || aligned16(variance)) &&
                     D <= 128 && !(logp == logits && addend);   // (in place with an addend: the scalar kernel's order)
    const dim3 grid(n_blocks(H, W), B);
    if (vec) {
        for_planes_per_lane(D, [&](auto rpl) {
            hipLaunchKernelGGL(dpv_reduce_ex_vec4_kernel<decltype(rpl)::value>, grid, dim3(256), 0, stream, logits, d_candi, D, HW, logp, depth, ex);
        });
    } else {
        hipLaunchKernelGGL(dpv_reduce_ex_scalar_kernel, grid, dim3(256), 0, stream, logits, d_candi, D, HW, logp, depth, ex);
    }
    return hipGetLastError();
}

hipError_t launch_dpv_expect(const float* dpv, const float* d_candi, int B, int D, int H, int W,
                             int bv_log, float* depth, hipStream_t stream) {
    const int HW = H * W;
    const bool vec = (HW % 4 == 0) && aligned16(dpv) && aligned16(depth);
    if (vec && D <= 128) {
        const dim3 grid(n_blocks(H, W), B);
        for_planes_per_lane(D, [&](auto rpl) {
            constexpr int RPL = decltype(rpl)::value;
            if (bv_log) hipLaunchKernelGGL((dpv_expect_vec4_kernel<true, RPL>), grid, dim3(256), 0, stream, dpv, d_candi, D, HW, depth);
            else hipLaunchKernelGGL((dpv_expect_vec4_kernel<false, RPL>), grid, dim3(256), 0, stream, dpv, d_candi, D, HW, depth);
        });
    } else if (vec) {
        dim3 grid((HW / 4 + 255) / 256, B);
        if (bv_log) hipLaunchKernelGGL((dpv_expect_kernel<true, 4>), grid, dim3(256), 0, stream, dpv, d_candi, D, HW, depth);
        else hipLaunchKernelGGL((dpv_expect_kernel<false, 4>), grid, dim3(256), 0, stream, dpv, d_candi, D, HW, depth);
    } else {
        const dim3 grid(n_blocks(H, W), B);
        if (bv_log) hipLaunchKernelGGL((dpv_expect_kernel<true, 1>), grid, dim3(256), 0, stream, dpv, d_candi, D, HW, depth);
        else hipLaunchKernelGGL((dpv_expect_kernel<false, 1>), grid, dim3(256), 0, stream, dpv, d_candi, D, HW, depth);
    }
    return hipGetLastError();
}

}  // namespace pdepth
