// The per-pixel arithmetic of the loss terms that more than one unit evaluates: the clamps, the relative difference and its
// derivatives, and the chain of the depth stereo consistency term (loss_terms.hip: forward and backward; scatter_det.hip: the
// order-independent sum of its src_depth gradient, through the same dsc_scatter), and the chain of the RGB stereo consistency term
// (loss_terms.hip: the L1 term; photo.hip: L1 and SSIM in one pass).  Every unit sees the same bits of every pixel.
#pragma once
#include <hip/hip_runtime.h>

#include "inverse_warp_math.hpp"

namespace pdepth {

namespace {

constexpr float FLOOR = 1e-3f;   // the clamp of every depth that enters a quotient (the warp's own: Z_FLOOR)

// torch.clamp(min=lo) / torch.clamp(0, 1): a NaN stays a NaN
__device__ __forceinline__ float clamp_min(float x, float lo) { return x < lo ? lo : x; }
__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
__device__ __forceinline__ float sign0(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }   // (NaN: 0)

// the relative difference clamp(|a - b| / |a + b|, 0, 1) and its two partial derivatives
struct RelDiff {
    float n, dd, q, diff;
};
__device__ __forceinline__ RelDiff rel_diff(float a, float b) {
    RelDiff r;
    r.n = fabsf(a - b);
    r.dd = fabsf(a + b);
    r.q = r.n / r.dd;
    r.diff = clamp01(r.q);
    return r;
}
// gd = dL / d diff -> (dL / da, dL / db)
__device__ __forceinline__ void rel_diff_grad(const RelDiff& r, float a, float b, float gd, float& ga, float& gb) {
    const float gq = (r.q >= 0.0f && r.q <= 1.0f) ? gd : 0.0f;
    const float gn = gq / r.dd;
    const float gdd = -gq * r.n / (r.dd * r.dd);
    const float s1 = sign0(a - b), s2 = sign0(a + b);
    ga = gn * s1 + gdd * s2;
    gb = gdd * s2 - gn * s1;
}

// ---- depth stereo consistency ---------------------------------------------------------------------------------------------------
struct DscArgs {
    const float* src;      // [B,H,W] source depth
    const float* tgt;      // [B,H,W] target depth
    const float* smask;    // [B,H,W] source mask
    const float* Kinv;     // [B,3,3]
    const float* proj;     // [B,3,4]
    const float* row;      // [B,4] | [1,4]: third row of the source-to-target pose
    const float* intr;     // [B,3,3]
    int row_stride;        // 4 | 0
    int H, W;
};

struct DscPixel {
    float m, tgt_m, got_m, a, b;
    int tap;
    float dmoved;          // d warped / d src[tap] (the source mask and the clamp's pass included); 0 without a tap
};

__device__ __forceinline__ DscPixel dsc_pixel(const DscArgs& g, int b, int pix) {
    const int H = g.H, W = g.W, HW = H * W;
    const int y = pix / W, x = pix - y * W;
    const float t = g.tgt[(size_t)b * HW + pix];
    const WarpSample q = warp_sample(g.Kinv + b * 9, g.proj + b * 12, x, y, t, H, W);
    DscPixel p;
    p.tap = nearest_tap(q, H, W);
    float warped = 0.0f;
    p.dmoved = 0.0f;
    if (p.tap >= 0) {
        // transform_dmap (utils/inverse_warp.py:212-253) of the source depth at the tap, times the source mask
        const float* K = g.intr + b * 9;
        const float* P = g.row + (size_t)b * g.row_stride;
        const int ty = p.tap / W, tx = p.tap - ty * W;
        const float xs = ((float)tx - K[2]) / K[0], ys = ((float)ty - K[5]) / K[4];
        const float zr = g.src[(size_t)b * HW + p.tap], sm = g.smask[(size_t)b * HW + p.tap];
        const float z = clamp_min(zr, FLOOR);
        const float moved = ((P[0] * (xs * z) + P[1] * (ys * z)) + P[2] * z) + P[3];
        warped = moved * sm;
        p.dmoved = zr >= FLOOR ? ((P[0] * xs + P[1] * ys) + P[2]) * sm : 0.0f;
    }
    p.m = (warp_valid(q) && y >= H / 3 && warped > 0.0f) ? 1.0f : 0.0f;
    p.tgt_m = t * p.m;
    p.got_m = warped * p.m;
    p.a = clamp_min(p.tgt_m, FLOOR);
    p.b = clamp_min(p.got_m, FLOOR);
    return p;
}


// the backward of one pixel: its own g_tgt, and the contribution v to g_src[tap] (tap < 0: none)
struct DscGrad {
    float g_tgt, v;
    int tap;
};
__device__ __forceinline__ DscGrad dsc_pixel_grad(const DscArgs& g, const float* __restrict__ count, const float* __restrict__ g_value,
                                                  int b, int pix) {
    const DscPixel p = dsc_pixel(g, b, pix);
    const RelDiff r = rel_diff(p.a, p.b);
    const float gd = (g_value[b] / count[b]) * p.m;
    float ga, gb;
    rel_diff_grad(r, p.a, p.b, gd, ga, gb);
    DscGrad d;
    d.g_tgt = p.tgt_m >= FLOOR ? ga * p.m : 0.0f;
    d.tap = p.tap;
    d.v = 0.0f;
    if (p.tap >= 0) {
        const float gw = p.got_m >= FLOOR ? gb * p.m : 0.0f;
        d.v = gw * p.dmoved;
    }
    return d;
}

// the contribution of one pixel to g_src [B,H,W] through a sink (fixed_accum.hpp); item0 = b H W
template <class Sink>
__device__ __forceinline__ void dsc_scatter(const DscGrad& d, long long item0, Sink& sink) {
    if (d.tap >= 0 && d.v != 0.0f) sink.add(item0 + d.tap, d.v);
}

// ---- RGB stereo consistency ----------------------------------------------------------------------------------------------------
// (loss_terms.hip: the L1 term; photo.hip: the same pixels with the SSIM distance of their windows)
struct RscArgs {
    const float* src;      // [B,3,H,W] source image
    const float* tgt;      // [B,3,H,W] target image
    const float* depth;    // [B,H,W] target depth
    const float* Kinv;
    const float* proj;
    int H, W;
};

// the position of a pixel's sample, its mask and its in-bounds taps: what the three channels share
struct RscSample {
    WarpSample q;
    float m;
    TapMask taps;
};
__device__ __forceinline__ RscSample rsc_sample(const RscArgs& g, int b, int pix, int x, int y) {
    const int H = g.H, W = g.W, HW = H * W;
    RscSample s;
    s.q = warp_sample(g.Kinv + b * 9, g.proj + b * 12, x, y, g.depth[(size_t)b * HW + pix], H, W);
    s.m = (warp_valid(s.q) && y >= H / 3) ? 1.0f : 0.0f;
    s.taps = tap_mask(s.q);
    return s;
}

// one channel of a pixel: x = warped m, y = tgt m, d = y - x, and the derivatives of warped with respect to the position
struct RscChannel {
    float x, y, d, gx, gy;
};
template <bool GRAD>
__device__ __forceinline__ RscChannel rsc_channel(const RscArgs& g, const RscSample& s, int b, int pix, int c) {
    const int W = g.W, HW = g.H * W;
    const WarpSample& q = s.q;
    const Texels v = load_texels(g.src + ((size_t)b * 3 + c) * HW + (q.y0 * W + q.x0), s.taps, W);
    const float warped = bilinear_value(q, v);
    RscChannel r;
    r.x = warped * s.m;
    r.y = g.tgt[((size_t)b * 3 + c) * HW + pix] * s.m;
    r.d = r.y - r.x;
    r.gx = GRAD ? bilinear_d_ix(q, v) : 0.0f;
    r.gy = GRAD ? bilinear_d_iy(q, v) : 0.0f;
    return r;
}

struct RscPixel {
    WarpSample q;
    float m;
    float x[3], y[3];      // warped_c m, tgt_c m
    float d[3];            // tgt_c m - warped_c m
    float gx[3], gy[3];    // d warped_c / d ix, d warped_c / d iy
};

template <bool GRAD>
__device__ __forceinline__ RscPixel rsc_pixel(const RscArgs& g, int b, int pix, int x, int y) {
    const RscSample s = rsc_sample(g, b, pix, x, y);
    RscPixel p;
    p.q = s.q;
    p.m = s.m;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const RscChannel r = rsc_channel<GRAD>(g, s, b, pix, c);
        p.x[c] = r.x;
        p.y[c] = r.y;
        p.d[c] = r.d;
        p.gx[c] = r.gx;
        p.gy[c] = r.gy;
    }
    return p;
}

// dL / d depth of pixel (x, y) from dL / d(ix, iy) of its sample: point_grad and the products behind it (the gradient of the
// camera point, of the depth); a non-finite position passes nothing
__device__ __forceinline__ float rsc_depth_grad(const RscArgs& g, int b, int x, int y, const WarpSample& q, float gix, float giy) {
    float out = 0.0f;
    if (q.finite) {
        const PointGrad gp = point_grad(q, gix, giy, g.H, g.W);
        const float* ki = g.Kinv + b * 9;
        const float* pr = g.proj + b * 12;
        const float fx = (float)x, fy = (float)y;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float gcam = __builtin_fmaf(pr[8 + j], gp.Z, __builtin_fmaf(pr[4 + j], gp.Y, pr[j] * gp.X));
            const float cam0 = __builtin_fmaf(ki[j * 3 + 2], 1.0f, __builtin_fmaf(ki[j * 3 + 1], fy, ki[j * 3 + 0] * fx));
            out = __builtin_fmaf(gcam, cam0, out);
        }
    }
    return out;
}

}  // namespace

}  // namespace pdepth
