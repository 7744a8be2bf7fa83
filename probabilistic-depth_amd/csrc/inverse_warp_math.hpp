// The per-pixel chain of inverse_warp (utils/inverse_warp.py:174-210: pixel2cam :26-40, cam2pixel :43-69, then the un-normalised
// sample position of F.grid_sample with align_corners=False), shared by the warp kernels of extras.hip and the loss terms of
// loss_terms.hip: both see the same bits of position, validity and tap, so a mask formed inside a loss kernel is the mask the
// warp's `valid` output and its nearest tap would have given.  Every object is built with -ffp-contract=off: the fmas below are
// the only ones.
#pragma once
#include <hip/hip_runtime.h>

namespace pdepth {

struct WarpSample {
    float X, Y, pz, Z;       // projected point, pz before the clamp
    float ix, iy;            // un-normalised sample position
    int x0, y0;              // top-left tap (clamped to [-2, size + 1])
    float nw, ne, sw, se;    // bilinear weights
    float w, e, n, s;
    bool finite, xi0, xi1, yi0, yi1;
    float xn, yn;
};

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
    q.Z = fmaxf(pc[2], 1e-3f);
    q.xn = 2.0f * (pc[0] / q.Z) / (float)(W - 1) - 1.0f;
    q.yn = 2.0f * (pc[1] / q.Z) / (float)(H - 1) - 1.0f;
    q.ix = __builtin_fmaf(q.xn + 1.0f, (float)W / 2.0f, -0.5f);
    q.iy = __builtin_fmaf(q.yn + 1.0f, (float)H / 2.0f, -0.5f);
    const float xf = floorf(q.ix), yf = floorf(q.iy);
    q.w = q.ix - xf; q.e = 1.0f - q.w; q.n = q.iy - yf; q.s = 1.0f - q.n;
    q.nw = q.s * q.e; q.ne = q.s * q.w; q.sw = q.n * q.e; q.se = q.n * q.w;
    q.finite = (q.ix == q.ix) && (q.iy == q.iy);
    q.x0 = (int)fminf(fmaxf(xf, -2.0f), (float)(W + 1)); q.y0 = (int)fminf(fmaxf(yf, -2.0f), (float)(H + 1));
    q.xi0 = q.x0 >= 0 && q.x0 < W; q.xi1 = q.x0 + 1 >= 0 && q.x0 + 1 < W;
    q.yi0 = q.y0 >= 0 && q.y0 < H; q.yi1 = q.y0 + 1 >= 0 && q.y0 + 1 < H;
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

}  // namespace pdepth
