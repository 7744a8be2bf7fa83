// The one body of the plane-sweep backward (the mathematics: header of sweep_bwd.hip).  sweep_bwd.hip (g_ref gather, g_src with
// float atomics) and sweep_bwd_det.hip (g_src as an integer sum) are wrappers around sweep_bwd_body<METRIC, GREF, Policy>: the
// tiles, the per-plane boxes, the plane groups, the direct-add fallback, the gather chain and the channel tail exist here and
// nowhere else, so the contributions of the two g_src paths are the same bit for bit by construction.
//
// A policy says what happens to a contribution:
//   Cell     element of the destination in global memory;
//   Stage    element of the LDS box image (the image is flushed with atomicAdd(Cell*, flush(Stage)));
//   BCC      channels per pass (grid z): BCC * BOX_CAP stage cells of LDS;
//   SCATTER  whether anything is scattered at all (false: no boxes, no groups, no LDS -- the g_ref gather);
//   add      one contribution to a cell, of the box image (LDS) or of the destination (global memory).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "fixed_accum.hpp"
#include "geometry.hpp"
#include "kernels.hpp"

namespace pdepth {
namespace sweep_bwd {

constexpr int BT = 16;            // tile edge (pixels)
constexpr int BTHREADS = BT * BT;
constexpr int BOX_CAP = 2048;     // texels of the LDS box image

struct NoScatter {   // g_ref alone
    using Cell = float;
    using Stage = float;
    static constexpr int BCC = 8;
    static constexpr bool SCATTER = false;
    __device__ __forceinline__ void add(float*, float) const {}
    static __device__ __forceinline__ float flush(float v) { return v; }
};
// The box image of the float path is double: a texel of the image takes every contribution of the group's planes, hundreds of
// terms at D = 128 and more, and their sum in float32 in the order of arrival was several times further from float64 than the
// reference's cascade sum.  In double the image is exact to 2^-53 per add; one rounding at the flush, then the
// few float adds of the groups and tiles that share a texel.
struct FloatAtomics {   // ds_add_f64 / global_atomic_add_f32: 4 * 2048 * 8 B = 64 KB
    using Cell = float;
    using Stage = double;
    static constexpr int BCC = 4;
    static constexpr bool SCATTER = true;
    __device__ __forceinline__ void add(double* q, float c) const { atomicAdd(q, (double)c); }   // the box image
    __device__ __forceinline__ void add(float* q, float c) const { atomicAdd(q, c); }            // a direct add
    static __device__ __forceinline__ float flush(double v) { return (float)v; }
};
struct IntegerSum {   // rn(2^S c) with ds_add_u64 / global_atomic_add_x2 (fixed_accum.hpp): 4 * 2048 * 8 B = 64 KB
    using Cell = unsigned long long;
    using Stage = unsigned long long;
    static constexpr int BCC = 4;   // (8: a 128 KB image, one workgroup per CU -- measured slower)
    static constexpr bool SCATTER = true;
    int S;   // the exponent of the workgroup's batch item
    __device__ __forceinline__ void add(unsigned long long* q, float c) const { fixed::det_add(q, c, S); }
    static __device__ __forceinline__ unsigned long long flush(unsigned long long v) { return v; }
};

// dynamic LDS of a launch: [4 waves][D][4] ints of boxes, then the box image
template <class Policy>
inline size_t lds_bytes(int D) {
    return Policy::SCATTER ? (size_t)16 * D * sizeof(int) + (size_t)Policy::BCC * BOX_CAP * sizeof(typename Policy::Stage) : 0;
}
template <class Policy>
inline dim3 grid(const SweepArgs& a) {
    return dim3(((a.W + BT - 1) / BT) * ((a.H + BT - 1) / BT), a.B, (a.C + Policy::BCC - 1) / Policy::BCC);
}

__device__ __forceinline__ int wave_min(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o, 64));
    return x;
}

// One workgroup (BTHREADS threads; blockIdx: tile, batch item, channel block) of the backward.  GREF: g_ref is gathered into
// gref [B,C,H,W]; Policy::SCATTER: the taps' contributions are added to dst [B,V,C,H,W] (zeroed by the launcher).  Both LDS
// pointers are derived here from the one dynamic-LDS symbol: the compiler sees which adds are LDS and which are global.
template <int METRIC, bool GREF, class Policy>
__device__ __forceinline__ void sweep_bwd_body(const SweepArgs& a, const float* __restrict__ gcost, float* __restrict__ gref,
                                               typename Policy::Cell* __restrict__ dst, const Policy pol) {
    using Cell = typename Policy::Cell;
    using Stage = typename Policy::Stage;
    constexpr int BCC = Policy::BCC;
    constexpr bool SCATTER = Policy::SCATTER;
    extern __shared__ unsigned long long sweep_bwd_lds[];
    int* box = reinterpret_cast<int*>(sweep_bwd_lds);         // [4 waves][D][4]: x min, x max, y min, y max of the wave's in-bounds taps of plane k
    Stage* img = reinterpret_cast<Stage*>(sweep_bwd_lds + 8 * a.D);   // [BCC][box area]
    const int tid = threadIdx.x;
    const int HW = a.H * a.W;
    const int b = blockIdx.y;
    const int tiles_x = (a.W + BT - 1) / BT;
    const int x = (blockIdx.x % tiles_x) * BT + (tid & (BT - 1));
    const int y = (blockIdx.x / tiles_x) * BT + (tid / BT);
    const bool live = x < a.W && y < a.H;
    const int p = live ? y * a.W + x : HW - 1;   // dead lanes shadow the last pixel and add nothing
    // H*W as a vector register: the per-channel offsets derived from it stay in vector registers (as scalars, eight 64-bit
    // channel offsets hoisted out of the plane loop spilled the scalar file)
    int hw_v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(hw_v) : "s"(HW));
    int w_v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(w_v) : "s"(a.W));

    const float cx = a.cxcy[b * 2 + 0];
    const float cy = a.cxcy[b * 2 + 1];
    const float half_w = (float)a.W / 2.0f;
    const float half_h = (float)a.H / 2.0f;
    const float r0 = a.rays[((size_t)b * 3 + 0) * HW + p];
    const float r1 = a.rays[((size_t)b * 3 + 1) * HW + p];
    const float r2 = a.rays[((size_t)b * 3 + 2) * HW + p];
    const float* refp = a.ref + (size_t)b * a.ref_bstride + p;
    const float* gk_p = gcost + (size_t)b * a.D * HW + p;
    float* grefp = gref + (size_t)b * a.C * HW + p;   // (unused without GREF)
    const float* srcb = a.src + (size_t)b * a.src_bstride;
    asm volatile("v_mov_b64 %0, %1" : "=v"(srcb) : "s"(srcb));   // (vector registers, as hw_v)
    const float gscale = (METRIC == 0 ? 2.0f : 1.0f) / a.sigma;

    for (int v = 0; v < a.V; ++v) {
        ViewXform xf;
        make_view_xform(a.K + b * 9, a.R + ((size_t)b * a.V + v) * 9, a.t + ((size_t)b * a.V + v) * 3, a.blas_mode, xf);
        float t2a, t2b, t2c;
        ray_term2(xf, r0, r1, r2, t2a, t2b, t2c);
        const float* srcv = srcb + (size_t)v * a.src_vstride;
        Cell* dstv = dst + ((size_t)b * a.V + v) * a.C * HW;   // (unused without SCATTER)

        if (SCATTER) {   // per-plane boxes of the tile's in-bounds taps
            __syncthreads();   // (the previous view's last reads of box[])
            for (int k = 0; k < a.D; ++k) {
                float ix, iy;
                plane_sample_pos(xf, t2a, t2b, t2c, a.d_candi[k], cx, cy, half_w, half_h, ix, iy);
                const Footprint f = make_footprint(ix, iy, a.W, a.H);
                const unsigned m = live ? f.mask : 0u;
                int x_lo = INT_MAX, x_hi = INT_MIN, y_lo = INT_MAX, y_hi = INT_MIN;
                if (m) {
                    x_lo = (m & 5u) ? f.x0 : f.x0 + 1;
                    x_hi = (m & 10u) ? f.x0 + 1 : f.x0;
                    y_lo = (m & 3u) ? f.y0 : f.y0 + 1;
                    y_hi = (m & 12u) ? f.y0 + 1 : f.y0;
                }
                x_lo = wave_min(x_lo); x_hi = wave_max(x_hi);
                y_lo = wave_min(y_lo); y_hi = wave_max(y_hi);
                if ((tid & 63) == 0) {
                    int* bk = box + 4 * ((tid >> 6) * a.D + k);
                    bk[0] = x_lo; bk[1] = x_hi; bk[2] = y_lo; bk[3] = y_hi;
                }
            }
            __syncthreads();
        }

        {   // this workgroup's BCC channels
            const int c0 = blockIdx.z * BCC;
            float rf[BCC];
            double gr[BCC];   // V D terms per pixel, one after another: in double (the float32 sum was noisier than the reference's cascade)
#pragma unroll
            for (int cc = 0; cc < BCC; ++cc) {
                rf[cc] = refp[min(c0 + cc, a.C - 1) * hw_v];
                gr[cc] = 0.0;
            }
            int k = 0;
            while (k < a.D) {   // groups of planes (workgroup-uniform)
                int k1 = a.D, bx0 = 0, by0 = 0, bw = 0, area = 0;
                bool staged = false;
                if (SCATTER) {
                    int ux0 = INT_MAX, ux1 = INT_MIN, uy0 = INT_MAX, uy1 = INT_MIN;
                    k1 = k;
                    while (k1 < a.D) {
                        int nx0 = ux0, nx1 = ux1, ny0 = uy0, ny1 = uy1;
                        for (int w = 0; w < BTHREADS / 64; ++w) {   // (an empty box is [INT_MAX, INT_MIN]: min / max leave it out)
                            const int* bk = box + 4 * (w * a.D + k1);
                            nx0 = min(nx0, bk[0]); nx1 = max(nx1, bk[1]);
                            ny0 = min(ny0, bk[2]); ny1 = max(ny1, bk[3]);
                        }
                        const long long na = nx0 <= nx1 ? (long long)(nx1 - nx0 + 1) * (ny1 - ny0 + 1) : 0;
                        if (na > BOX_CAP) break;
                        ux0 = nx0; ux1 = nx1; uy0 = ny0; uy1 = ny1;
                        ++k1;
                    }
                    if (k1 == k) {
                        k1 = k + 1;   // this plane's box alone does not fit: direct adds
                    } else if (ux0 <= ux1) {
                        staged = true;
                        bx0 = ux0; by0 = uy0; bw = ux1 - ux0 + 1; area = bw * (uy1 - uy0 + 1);
                        #pragma unroll 1
                        for (int i = tid; i < BCC * area; i += BTHREADS) img[i] = Stage(0);
                        __syncthreads();
                    } else if (!GREF) {
                        k = k1;   // a run of planes without an in-bounds tap: nothing to add (the g_ref gather needs every plane)
                        continue;
                    }
                }
                for (int kk = k; kk < k1; ++kk) {
                    float ix, iy;
                    plane_sample_pos(xf, t2a, t2b, t2c, a.d_candi[kk], cx, cy, half_w, half_h, ix, iy);
                    const Footprint f = make_footprint(ix, iy, a.W, a.H);
                    const unsigned m = live ? f.mask : 0u;
                    const float g = live ? gk_p[(size_t)kk * HW] : 0.0f;
                    const float coef = g * gscale;
                    const float* s00 = srcv + (f.y0 * a.W + f.x0);   // (texel of channel 0: co below adds the channel)
                    const int lo = staged ? (f.y0 - by0) * bw + (f.x0 - bx0) : 0;
                    float rr[BCC];
#pragma unroll
                    for (int cc = 0; cc < BCC; ++cc) {   // gather: e and the gradient of the cost term, channel c0 + cc
                        const int co = min(c0 + cc, a.C - 1) * hw_v;   // (past the last channel: a copy of it, weighted 0)
                        const float* s = s00 + co;
                        const float vnw = (f.mask & 1u) ? s[0] : 0.0f;
                        const float vne = (f.mask & 2u) ? s[1] : 0.0f;
                        const float vsw = (f.mask & 4u) ? s[w_v] : 0.0f;
                        const float vse = (f.mask & 8u) ? s[w_v + 1] : 0.0f;
                        float val = vnw * f.nw;
                        val = __builtin_fmaf(vne, f.ne, val);
                        val = __builtin_fmaf(vsw, f.sw, val);
                        val = __builtin_fmaf(vse, f.se, val);
                        const float e = val - rf[cc];
                        const float r = METRIC == 0 ? coef * e : (e > 0.0f ? coef : (e < 0.0f ? -coef : 0.0f));
                        rr[cc] = c0 + cc < a.C ? r : 0.0f;
                        gr[cc] = gr[cc] - (double)rr[cc];
                    }
                    if (!SCATTER || !m) continue;   // (no in-bounds tap: nothing to add)
                    // (expect: the direct adds are laid out behind the plane loop, not in the middle of it -- 1 % of the integer scatter)
                    if (__builtin_expect(staged, 1)) {   // (rows of the image past the last channel are never flushed)
                        Stage* q = img + lo;
#pragma unroll
                        for (int cc = 0; cc < BCC; ++cc) {
                            if (m & 1u) pol.add(q, f.nw * rr[cc]);
                            if (m & 2u) pol.add(q + 1, f.ne * rr[cc]);
                            if (m & 4u) pol.add(q + bw, f.sw * rr[cc]);
                            if (m & 8u) pol.add(q + bw + 1, f.se * rr[cc]);
                            q += area;
                        }
                    } else {
                        Cell* q = dstv + (c0 * HW + f.y0 * a.W + f.x0);
                        #pragma unroll 1   // (the rare path: rolled, as small as it can be)
                        for (int cc = 0; cc < BCC && c0 + cc < a.C; ++cc) {
                            if (m & 1u) pol.add(q, f.nw * rr[cc]);
                            if (m & 2u) pol.add(q + 1, f.ne * rr[cc]);
                            if (m & 4u) pol.add(q + w_v, f.sw * rr[cc]);
                            if (m & 8u) pol.add(q + w_v + 1, f.se * rr[cc]);
                            q += hw_v;
                        }
                    }
                }
                if (staged) {   // the group's box image -> dst, one texel per lane, lanes along the box rows
                    __syncthreads();
                    const int nc = min(BCC, a.C - c0);
                    #pragma unroll 1
                    for (int i = tid; i < nc * area; i += BTHREADS) {
                        const int cc = i / area, rr = i - cc * area;
                        const int ry = rr / bw, rx = rr - ry * bw;
                        const Stage val = img[i];
                        if (val != Stage(0)) atomicAdd(dstv + (size_t)(c0 + cc) * HW + (by0 + ry) * a.W + (bx0 + rx), Policy::flush(val));
                    }
                    __syncthreads();   // (the next group zeroes the image)
                }
                k = k1;
            }
            if (GREF && live) {
#pragma unroll
                for (int cc = 0; cc < BCC; ++cc) {
                    if (c0 + cc < a.C) {
                        float* o = grefp + (c0 + cc) * hw_v;
                        *o = v == 0 ? (float)gr[cc] : *o + (float)gr[cc];   // views in order: reproducible
                    }
                }
            }
        }
    }
}

}  // namespace sweep_bwd
}  // namespace pdepth
