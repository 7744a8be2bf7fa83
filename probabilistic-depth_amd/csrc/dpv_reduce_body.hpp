// The arithmetic of the DPV reductions, forward and backward, once: dpv.hip / dpv_bwd.hip instantiate it on fp32 volumes,
// dpv_half.hip on fp16 / bf16 logits (and prob, and g_logits).  An element type enters at a load (widened to fp32, exact) or at
// a store (rounded to nearest-even from the fp32 value) and nowhere else: the operations between are the same ones in the same
// order, so with -ffp-contract=off a half-precision call gives the bits of the fp32 call on the widened input.
#pragma once
#include <hip/hip_runtime.h>

#include "dpv_lanes.hpp"

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
// the same with the addend in the logits' element type X and prob in P (pdepth_dpv_reduce_ex_lp)
template <typename X, typename P>
struct DpvExtrasAs {
    const X* addend;
    P* prob;
    float* variance;
    float* quarter;
    int W;
};

// The log-softmax sweep of a lane's RPL planes + the expectation; EX: with the extras (compiled out of the plain kernel).
template <int RPL, bool EX, typename X, typename EXT>
__device__ __forceinline__ void dpv_reduce_lanes(const X* __restrict__ x, const float* __restrict__ dc, int D, int HW,
                                                 float* logp, float* __restrict__ depth, const EXT& ex) {
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

// sum_k term(k) over the planes of one pixel.  LANES = false: ascending k, the any-shape kernels' own order.  LANES = true:
// the order of the wave layout seen from one pixel -- four partial sums over the planes k = g + 4 i in ascending i, combined
// as group_sum does, (s0 + s1) + (s2 + s3) -- for a volume only its base address keeps out of the wave layout.
template <bool LANES, typename F>
__device__ __forceinline__ float plane_sum(int D, F&& term) {
    if constexpr (!LANES) {
        float s = 0.f;
        for (int k = 0; k < D; ++k) s += term(k);
        return s;
    } else {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int k = 0; k < D; k += 4) {
            s0 += term(k);
            if (k + 1 < D) s1 += term(k + 1);
            if (k + 2 < D) s2 += term(k + 2);
            if (k + 3 < D) s3 += term(k + 3);
        }
        return (s0 + s1) + (s2 + s3);
    }
}

// The extended reduction of one pixel per thread: any D, any H, W, any base address (re-reads hit L2).
template <bool LANES, typename X, typename EXT>
__device__ __forceinline__ void dpv_reduce_ex_pixel(const X* x, const float* __restrict__ dc, int D, int HW, float* logp,
                                                    float* __restrict__ depth, const EXT& ex) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const size_t off = (size_t)b * D * HW + pix;
    auto at = [&](int k) { return widen(x[off + (size_t)k * HW]) + (ex.addend ? widen(ex.addend[off + (size_t)k * HW]) : 0.0f); };
    float m = -INFINITY;
    for (int k = 0; k < D; ++k) m = fmaxf(m, at(k));
    const float s = plane_sum<LANES>(D, [&](int k) { return expf(at(k) - m); });
    const float ls = logf(s);
    const int py = pix / ex.W, px = pix - py * ex.W, Wq = ex.W >> 2, Hq = (HW / ex.W) >> 2;
    const bool qpix = ex.quarter && (py & 3) == 0 && (px & 3) == 0 && (py >> 2) < Hq && (px >> 2) < Wq;
    // (logp may alias logits: nothing is read again after this sweep unless variance)
    const float e = plane_sum<LANES>(D, [&](int k) {
        const float lp = (at(k) - m) - ls;
        return dc[k] * expf(lp);
    });
    using P = std::remove_pointer_t<decltype(ex.prob)>;
    const float var = plane_sum<LANES>(D, [&](int k) {
        const float lp = (at(k) - m) - ls, p = expf(lp), dd = dc[k] - e;
        if (ex.prob) ex.prob[off + (size_t)k * HW] = narrow<P>(p);
        if (qpix) ex.quarter[((size_t)b * D + k) * Hq * Wq + (size_t)(py >> 2) * Wq + (px >> 2)] = lp;
        return (dd * dd) * p;
    });
    if (logp)
        for (int k = 0; k < D; ++k) logp[off + (size_t)k * HW] = (at(k) - m) - ls;   // last: logp may alias logits
    if (depth) depth[(size_t)b * HW + pix] = e;
    if (ex.variance) ex.variance[(size_t)b * HW + pix] = var;
}

// Backward of the reductions for one pixel per thread, planes ascending (dpv_bwd.hip); GX: the element type g_x is stored in,
// GP: the one g_prob is read in.
template <typename GX, typename GP>
__device__ __forceinline__ void dpv_reduce_bwd_pixel(const float* __restrict__ logp, const float* __restrict__ dc, int D, int HW,
                                                     const float* __restrict__ g_logp, const GP* __restrict__ g_prob,
                                                     const float* __restrict__ g_depth, GX* __restrict__ g_x) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= HW) return;
    const size_t b = blockIdx.y;
    const size_t base = b * D * HW + pix;
    const float gd = g_depth ? g_depth[b * HW + pix] : 0.0f;
    float sum = 0.0f;
    for (int k = 0; k < D; ++k) {
        const size_t i = base + (size_t)k * HW;
        const float p = expf(logp[i]);
        float G = g_logp ? g_logp[i] : 0.0f;
        G = G + p * ((g_prob ? widen(g_prob[i]) : 0.0f) + gd * dc[k]);
        sum = sum + G;
    }
    for (int k = 0; k < D; ++k) {
        const size_t i = base + (size_t)k * HW;
        const float p = expf(logp[i]);
        float G = g_logp ? g_logp[i] : 0.0f;
        G = G + p * ((g_prob ? widen(g_prob[i]) : 0.0f) + gd * dc[k]);
        g_x[i] = narrow<GX>(G - p * sum);
    }
}

}  // namespace pdepth
