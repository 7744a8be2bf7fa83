// The per-pixel chain of inverse_warp (utils/inverse_warp.py:174-210: pixel2cam :26-40, cam2pixel :43-69, then the un-normalised
// sample position of F.grid_sample with align_corners=False), shared by the warp kernels of inverse_warp.hip and the loss terms of
// loss_terms.hip: both see the same bits of position, validity and tap, so a mask formed inside a loss kernel is the mask the
// warp's `valid` output and its nearest tap would have given.  Every object is built with -ffp-contract=off: the fmas below are
// the only ones.
//
// Behind the position: the in-bounds taps (TapMask), the masked load of a channel's four texels, their bilinear value and its two
// derivatives with respect to the position, the gradient of the projected point, and the scatter of an upstream gradient to the
// taps through a sink (fixed_accum.hpp: FloatAtomics, MaxOfAbs, IntegerSum) -- each once, for the forward and backward kernels of
// inverse_warp.hip, the rsc term of loss_terms.hip, the integer sums of scatter_det.hip and the range map of occlusion.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace pdepth {

constexpr float Z_FLOOR = 1e-3f;   // cam2pixel's clamp of the projected depth

struct WarpSample {
    float X, Y, pz, Z;       // projected point, pz before the clamp
    float ix, iy;            // un-normalised sample position
    int x0, y0;              // top-left tap (clamped to [-2, size + 1])
    float nw, ne, sw, se;    // bilinear weights
    float w, e, n, s;
    bool finite, xi0, xi1, yi0, yi1;
    float xn, yn;
};

// the bilinear footprint of the un-normalised position (q.ix, q.iy): fractions, weights, the top-left tap and which taps lie inside
__device__ __forceinline__ void place_taps(WarpSample& q, int H, int W) {
    const float xf = floorf(q.ix), yf = floorf(q.iy);
    q.w = q.ix - xf; q.e = 1.0f - q.w; q.n = q.iy - yf; q.s = 1.0f - q.n;
    q.nw = q.s * q.e; q.ne = q.s * q.w; q.sw = q.n * q.e; q.se = q.n * q.w;
    q.finite = (q.ix == q.ix) && (q.iy == q.iy);
    q.x0 = (int)fminf(fmaxf(xf, -2.0f), (float)(W + 1)); q.y0 = (int)fminf(fmaxf(yf, -2.0f), (float)(H + 1));
    q.xi0 = q.x0 >= 0 && q.x0 < W; q.xi1 = q.x0 + 1 >= 0 && q.x0 + 1 < W;
    q.yi0 = q.y0 >= 0 && q.y0 < H; q.yi1 = q.y0 + 1 >= 0 && q.y0 + 1 < H;
}

// a sample at a given un-normalised position (the range map of occlusion.hip, whose positions arrive as data): the footprint
// alone, the projected point left at 0
__device__ __forceinline__ WarpSample sample_at(float ix, float iy, int H, int W) {
    WarpSample q{};
    q.ix = ix; q.iy = iy;
    place_taps(q, H, W);
    return q;
}

__device__ __forceinline__ WarpSample warp_sample(const float* __restrict__ ki, const float* __restrict__ pr, int x, int y,
                                                   float d, int H, int W) {
    WarpSample q;
    const float fx = (float)x, fy = (float)y;
    float cam[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        cam[i] = __builtin_fmaf(ki[i * 3 + 2], 1.0f, __builtin_fmaf(ki[i * 3 + 1], fy, ki[i * 3 + 0] * fx)) * d;
    float pc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        pc[i] = __builtin_fmaf(pr[i * 4 + 2], cam[2], __builtin_fmaf(pr[i * 4 + 1], cam[1], pr[i * 4 + 0] * cam[0])) + pr[i * 4 + 3];
    q.X = pc[0]; q.Y = pc[1]; q.pz = pc[2];
    q.Z = fmaxf(pc[2], Z_FLOOR);
    q.xn = 2.0f * (pc[0] / q.Z) / (float)(W - 1) - 1.0f;
    q.yn = 2.0f * (pc[1] / q.Z) / (float)(H - 1) - 1.0f;
    q.ix = __builtin_fmaf(q.xn + 1.0f, (float)W / 2.0f, -0.5f);
    q.iy = __builtin_fmaf(q.yn + 1.0f, (float)H / 2.0f, -0.5f);
    place_taps(q, H, W);
    return q;
}

// the `valid` output of inverse_warp: both normalised coordinates inside [-1, 1]
__device__ __forceinline__ bool warp_valid(const WarpSample& q) { return fmaxf(fabsf(q.xn), fabsf(q.yn)) <= 1.0f; }

// nearest tap of grid_sample(mode='nearest'): round half to even of the un-normalised position; -1 = outside / NaN
__device__ __forceinline__ int nearest_tap(const WarpSample& q, int H, int W) {
    if (!q.finite) return -1;
    const float rx = rintf(q.ix), ry = rintf(q.iy);
    if (!(rx >= 0.0f && rx < (float)W && ry >= 0.0f && ry < (float)H)) return -1;
    return (int)ry * W + (int)rx;
}

// ---- the bilinear footprint ---------------------------------------------------------------------------------------------------------
// the in-bounds taps of a sample; a non-finite position has none
struct TapMask {
    bool nw, ne, sw, se;
    __device__ __forceinline__ bool any() const { return nw || ne || sw || se; }
};
__device__ __forceinline__ TapMask tap_mask(const WarpSample& q) {
    return {q.finite && q.xi0 && q.yi0, q.finite && q.xi1 && q.yi0, q.finite && q.xi0 && q.yi1, q.finite && q.xi1 && q.yi1};
}

// a channel's four texels, zeros outside; p: the channel's element (y0, x0), which may lie outside
struct Texels {
    float nw, ne, sw, se;
};
__device__ __forceinline__ Texels load_texels(const float* __restrict__ p, const TapMask& m, int W) {
    return {m.nw ? p[0] : 0.0f, m.ne ? p[1] : 0.0f, m.sw ? p[W] : 0.0f, m.se ? p[W + 1] : 0.0f};
}

__device__ __forceinline__ float bilinear_value(const WarpSample& q, const Texels& v) {
    return __builtin_fmaf(v.se, q.se, __builtin_fmaf(v.sw, q.sw, __builtin_fmaf(v.ne, q.ne, v.nw * q.nw)));
}
// d value / d ix = (ne - nw) s + (se - sw) n,  d value / d iy = (sw - nw) e + (se - ne) w
__device__ __forceinline__ float bilinear_d_ix(const WarpSample& q, const Texels& v) {
    return __builtin_fmaf(v.se - v.sw, q.n, (v.ne - v.nw) * q.s);
}
__device__ __forceinline__ float bilinear_d_iy(const WarpSample& q, const Texels& v) {
    return __builtin_fmaf(v.se - v.ne, q.w, (v.sw - v.nw) * q.e);
}

// dL / d(X, Y, Z) of the projected point from dL / d(ix, iy), for a finite position:
// ix = ((xn + 1) W - 1) / 2, xn = 2 (X / Z) / (W - 1) - 1, Z = max(pz, Z_FLOOR) (the clamp passes the gradient for pz >= Z_FLOOR)
struct PointGrad {
    float X, Y, Z;
};
__device__ __forceinline__ PointGrad point_grad(const WarpSample& q, float gix, float giy, int H, int W) {
    const float gxn = gix * ((float)W / 2.0f), gyn = giy * ((float)H / 2.0f);
    PointGrad g;
    g.X = gxn * 2.0f / ((float)(W - 1) * q.Z);
    g.Y = gyn * 2.0f / ((float)(H - 1) * q.Z);
    g.Z = q.pz >= Z_FLOOR ? -(g.X * q.X + g.Y * q.Y) / q.Z : 0.0f;
    return g;
}

// ---- grad_img: the scatter of the upstream gradient to the taps -------------------------------------------------------------------------
// Sink: add(long long at, float q), `at` an element of the contiguous [B,C,H,W] gradient.  As ATen's grid_sampler_2d backward: an
// in-bounds tap receives g w even when w == 0, an out-of-bounds tap nothing.
// one channel's g to the in-bounds taps; at: the channel's element (y0, x0), which may lie outside (then unused)
template <class Sink>
__device__ __forceinline__ void scatter_taps(const WarpSample& q, const TapMask& m, long long at, int W, float g, Sink& sink) {
    const float qnw = g * q.nw, qne = g * q.ne, qsw = g * q.sw, qse = g * q.se;
    if (m.nw) sink.add(at, qnw);
    if (m.ne) sink.add(at + 1, qne);
    if (m.sw) sink.add(at + W, qsw);
    if (m.se) sink.add(at + W + 1, qse);
}

// one sample over its C channels: g at the nearest tap (MODE 1) / g w_t at the in-bounds taps (MODE 0).  gb: the sample's element
// of channel 0 of grad_out [B,C,H,W]; image0 = b C H W; a sample that is not live adds nothing.
template <int MODE, class Sink>
__device__ __forceinline__ void scatter_sample(const WarpSample& q, bool live, const float* __restrict__ gb, long long image0, int C,
                                               int H, int W, Sink& sink) {
    const int HW = H * W;
    if (MODE == 1) {
        const int tap = live ? nearest_tap(q, H, W) : -1;
        if (tap >= 0)
            for (int c = 0; c < C; ++c) sink.add(image0 + (long long)c * HW + tap, gb[(size_t)c * HW]);
    } else {
        const TapMask t = tap_mask(q);
        const TapMask m{live && t.nw, live && t.ne, live && t.sw, live && t.se};
        if (m.any()) {
            const long long at = image0 + (q.y0 * W + q.x0);
            for (int c = 0; c < C; ++c) scatter_taps(q, m, at + (long long)c * HW, W, gb[(size_t)c * HW], sink);
        }
    }
}

}  // namespace pdepth
