// The per-sample chain of warp_feature, shared by its forward (warp.hip) and its backward (warp_bwd.hip): the homography terms of a
// (batch item, view), the ray term of a pixel, the sample position of a plane (the divide chain a.fast_div selects) and the bilinear
// footprint -- the helpers of geometry.hpp, called in one place, so that the taps and weights the backward scatters through are the
// forward's bit for bit.  The launchers share the grid as well: (pixel blocks of 256, V * plane chunks, B).
#pragma once
#include <hip/hip_runtime.h>

#include "geometry.hpp"
#include "kernels.hpp"

namespace pdepth {
namespace warp_sample {

// what is fixed for a thread: one pixel of one view of one batch item
struct PixelChain {
    ViewXform xf;
    float t2a, t2b, t2c;   // (K @ R) @ ray
    float cx, cy, rcx, rcy, half_w, half_h;
};

__device__ __forceinline__ void make_pixel_chain(const SweepArgs& a, int b, int v, int pix, PixelChain& c) {
    const int HW = a.H * a.W;
    make_view_xform(a.K + b * 9, a.R + ((size_t)b * a.V + v) * 9, a.t + ((size_t)b * a.V + v) * 3, a.blas_mode, c.xf);
    ray_term2(c.xf, a.rays[((size_t)b * 3 + 0) * HW + pix], a.rays[((size_t)b * 3 + 1) * HW + pix],
              a.rays[((size_t)b * 3 + 2) * HW + pix], c.t2a, c.t2b, c.t2c);
    c.cx = a.cxcy[b * 2 + 0];
    c.cy = a.cxcy[b * 2 + 1];
    c.half_w = (float)a.W / 2.0f;
    c.half_h = (float)a.H / 2.0f;
    c.rcx = refined_rcp(c.cx);
    c.rcy = refined_rcp(c.cy);
}

// the footprint of the thread's pixel on plane k
__device__ __forceinline__ Footprint plane_footprint(const SweepArgs& a, const PixelChain& c, int k) {
    float ix, iy;
    // (the fast divide chain is bit-identical to the IEEE one wherever a tap can land inside the image: geometry.hpp)
    if (a.fast_div) plane_sample_pos_fast(c.xf, c.t2a, c.t2b, c.t2c, a.d_candi[k], c.cx, c.cy, c.rcx, c.rcy, c.half_w, c.half_h, ix, iy);
    else plane_sample_pos(c.xf, c.t2a, c.t2b, c.t2c, a.d_candi[k], c.cx, c.cy, c.half_w, c.half_h, ix, iy);
    return make_footprint(ix, iy, a.W, a.H);
}

// grid (pixel blocks, V * nchunk, B): a thread takes planes chunk, chunk + nchunk, ... of its pixel -- on the model's small
// maps (64x128) one thread per pixel walking all D planes leaves the chip a block per CU and a chain of dependent gathers.
inline int plane_chunks(const SweepArgs& a) {
    const int pixblocks = (a.H * a.W + 255) / 256;
    long long nchunk = 2048 / ((long long)pixblocks * a.V * a.B);   // at least ~8 blocks per CU
    nchunk = nchunk < 1 ? 1 : nchunk > 16 ? 16 : nchunk;
    if (nchunk > a.D) nchunk = a.D;
    if ((long long)a.V * nchunk > 65535) nchunk = 1;
    return (int)nchunk;
}
inline dim3 grid(const SweepArgs& a, int nchunk) { return dim3((a.H * a.W + 255) / 256, a.V * nchunk, a.B); }

}  // namespace warp_sample
}  // namespace pdepth
