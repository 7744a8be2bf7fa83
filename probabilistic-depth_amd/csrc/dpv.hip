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
#include "kernels.hpp"

namespace pdepth {

// Extras of the extended reduction (pdepth_dpv_reduce_ex_f32): the same single pass with optional outputs, all from the
// registers that already hold the column --
//   addend   : x = logits + addend before the softmax   (feedback update log_softmax(BV_cur + BV_resi), models.py:694)
//   prob     : exp(logp), the decoder's input            (models.py:697 torch.exp(BV_cur_upd), :651)
//   variance : sum_k (d_k - E[d])^2 p_k                   (trainer/default_trainer.py:333-336)
//   quarter  : logp at every 4th row and column, [B,D,H/4,W/4] = F.interpolate(logp, scale_factor=0.25,
//              mode='nearest'), the next frame's prev_output (trainer/default_trainer.py:221)
struct DpvExtras {
    const float* addend;
    float* prob;
    float* variance;
    float* quarter;
    int W;
};

// The log-softmax sweep of a lane's RPL planes + the expectation; EX: with the extras (compiled out of the plain kernel).
template <int RPL, bool EX>
__device__ __forceinline__ void dpv_reduce_lanes(const float* __restrict__ x, const float* __restrict__ dc, int D, int HW,
                                                 float* logp, float* __restrict__ depth, const DpvExtras& ex) {
    const QuadLane L = quad_lane(D, HW);
    const int g = L.g, b = L.b;
    const bool live = L.live;
    float4 v[RPL];
    load_planes(v, x, L, 0, D, HW, -INFINITY, true, EX ? ex.addend : nullptr);
    float4 m = v[0];
#pragma unroll
    for (int i = 1; i < RPL; ++i) {
        m.x = fmaxf(m.x, v[i].x); m.y = fmaxf(m.y, v[i].y); m.z = fmaxf(m.z, v[i].z); m.w = fmaxf(m.w, v[i].w);
    }
    m = group_max(m);
    float4 sum = splat4(0.f);
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
        if (g + 4 * i < D) {
            v[i].x -= m.x; v[i].y -= m.y; v[i].z -= m.z; v[i].w -= m.w;
            sum.x += expf(v[i].x); sum.y += expf(v[i].y); sum.z += expf(v[i].z); sum.w += expf(v[i].w);
        }
    }
    sum = group_sum(sum);
    const float4 ls = make_float4(logf(sum.x), logf(sum.y), logf(sum.z), logf(sum.w));
    float4 e = splat4(0.f);
    // quarter-resolution copy: this lane's first pixel, when its row is a multiple of 4 (W % 4 == 0: a quad never
    // straddles rows and starts at a column that is a multiple of 4)
    int py = 0, pxq = 0, Wq = 0, Hq = 0;
    bool qrow = false;
    if (EX) {
        const int pix = L.q * 4;
        py = pix / ex.W, pxq = (pix - py * ex.W) >> 2;
        Wq = ex.W >> 2, Hq = (HW / ex.W) >> 2;
        qrow = ex.quarter && live && (py & 3) == 0 && (py >> 2) < Hq && pxq < Wq;
    }
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
        const int k = g + 4 * i;
        if (k < D) {
            const float4 lp = make_float4(v[i].x - ls.x, v[i].y - ls.y, v[i].z - ls.z, v[i].w - ls.w);
            const float4 p = make_float4(expf(lp.x), expf(lp.y), expf(lp.z), expf(lp.w));
            if (EX) v[i] = p;   // (kept for the variance sweep)
            if (live) {
                if (logp) store_nt(logp + L.off + (size_t)k * HW, lp);
                if (EX && ex.prob) store_nt(ex.prob + L.off + (size_t)k * HW, p);
                if (EX && qrow) ex.quarter[((size_t)b * D + k) * Hq * Wq + (size_t)(py >> 2) * Wq + pxq] = lp.x;
            }
            expect_add<false>(e, dc[k], p);
        }
    }
    e = group_sum(e);
    if (depth && live && g == 0) *reinterpret_cast<float4*>(depth + L.poff) = e;
    if (EX && ex.variance) {   // second sweep over the registers: sum_k (d_k - mean)^2 p_k with the mean just formed
        float4 var = splat4(0.f);
#pragma unroll
        for (int i = 0; i < RPL; ++i) {
            const int k = g + 4 * i;
            if (k < D) {
                const float dk = dc[k];
                const float4 dd = make_float4(dk - e.x, dk - e.y, dk - e.z, dk - e.w);
                var.x += (dd.x * dd.x) * v[i].x; var.y += (dd.y * dd.y) * v[i].y;
                var.z += (dd.z * dd.z) * v[i].z; var.w += (dd.w * dd.w) * v[i].w;
            }
        }
        var = group_sum(var);
        if (live && g == 0) *reinterpret_cast<float4*>(ex.variance + L.poff) = var;
    }
}

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
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const size_t off = (size_t)b * D * HW + pix;
    auto at = [&](int k) { return x[off + (size_t)k * HW] + (ex.addend ? ex.addend[off + (size_t)k * HW] : 0.0f); };
    float m = -INFINITY;
    for (int k = 0; k < D; ++k) m = fmaxf(m, at(k));
    float s = 0.f;
    for (int k = 0; k < D; ++k) s += expf(at(k) - m);
    const float ls = logf(s);
    const int py = pix / ex.W, px = pix - py * ex.W, Wq = ex.W >> 2, Hq = (HW / ex.W) >> 2;
    const bool qpix = ex.quarter && (py & 3) == 0 && (px & 3) == 0 && (py >> 2) < Hq && (px >> 2) < Wq;
    float e = 0.f;
    for (int k = 0; k < D; ++k) {   // (logp may alias logits: nothing is read again after this sweep unless variance)
        const float lp = (at(k) - m) - ls;
        e += dc[k] * expf(lp);
    }
    float var = 0.f;
    for (int k = 0; k < D; ++k) {
        const float lp = (at(k) - m) - ls, p = expf(lp), dd = dc[k] - e;
        var += (dd * dd) * p;
        if (ex.prob) ex.prob[off + (size_t)k * HW] = p;
        if (qpix) ex.quarter[((size_t)b * D + k) * Hq * Wq + (size_t)(py >> 2) * Wq + (px >> 2)] = lp;
    }
    if (logp)
        for (int k = 0; k < D; ++k) logp[off + (size_t)k * HW] = (at(k) - m) - ls;   // last: logp may alias logits
    if (depth) depth[(size_t)b * HW + pix] = e;
    if (ex.variance) ex.variance[(size_t)b * HW + pix] = var;
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
