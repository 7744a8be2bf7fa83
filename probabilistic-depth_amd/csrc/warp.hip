// Diagonal feature warp + coordinate dump.
//
// warp_feature (warping/homography.py:137-168): the reference warps every channel of a
// view with every depth plane ([D,C,h,w]) and keeps only the diagonal [i,i] -- channel i
// sampled with plane i.  This kernel samples exactly that diagonal: one bilinear gather per
// (view, plane, pixel), 1/D of the reference's work, 8*h*w*V*D algorithmic bytes.
#include <hip/hip_runtime.h>

#include "geometry.hpp"
#include "kernels.hpp"
#include "warp_sample.hpp"

namespace pdepth {

using namespace warp_sample;

// grid (pixel blocks, V * nchunk, B): a thread takes planes chunk, chunk + nchunk, ... of its pixel (warp_sample.hpp, with the
// per-sample chain the backward of warp_bwd.hip shares)
__global__ __launch_bounds__(256) void warp_feature_kernel(SweepArgs a, int nchunk, float* __restrict__ out) {
    const int HW = a.H * a.W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int v = blockIdx.y / nchunk, chunk = blockIdx.y - v * nchunk;
    const int b = blockIdx.z;
    PixelChain c;
    make_pixel_chain(a, b, v, pix, c);
    const float* srcv = a.src + (size_t)b * a.src_bstride + (size_t)v * a.src_vstride;
    float* o = out + (((size_t)b * a.V + v) * a.D) * HW + pix;
    for (int k = chunk; k < a.D; k += nchunk) {
        const Footprint f = plane_footprint(a, c, k);
        const float* s = srcv + (size_t)k * HW + (f.y0 * a.W + f.x0);
        const float vnw = (f.mask & 1u) ? s[0] : 0.0f;
        const float vne = (f.mask & 2u) ? s[1] : 0.0f;
        const float vsw = (f.mask & 4u) ? s[a.W] : 0.0f;
        const float vse = (f.mask & 8u) ? s[a.W + 1] : 0.0f;
        float val = vnw * f.nw;
        val = __builtin_fmaf(vne, f.ne, val);
        val = __builtin_fmaf(vsw, f.sw, val);
        val = __builtin_fmaf(vse, f.se, val);
        o[(size_t)k * HW] = val;
    }
}

__global__ __launch_bounds__(256) void sample_coords_kernel(SweepArgs a, float* __restrict__ oix,
                                                            float* __restrict__ oiy) {
    const int HW = a.H * a.W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int v = blockIdx.y;
    const int b = blockIdx.z;
    PixelChain c;
    make_pixel_chain(a, b, v, pix, c);
    const size_t base = (((size_t)b * a.V + v) * a.D) * HW + pix;
    for (int k = 0; k < a.D; ++k) {
        float ix, iy;
        if (a.fast_div) plane_sample_pos_fast(c.xf, c.t2a, c.t2b, c.t2c, a.d_candi[k], c.cx, c.cy, c.rcx, c.rcy, c.half_w, c.half_h, ix, iy);
        else plane_sample_pos(c.xf, c.t2a, c.t2b, c.t2c, a.d_candi[k], c.cx, c.cy, c.half_w, c.half_h, ix, iy);
        oix[base + (size_t)k * HW] = ix;
        oiy[base + (size_t)k * HW] = iy;
    }
}

hipError_t launch_warp_feature(const SweepArgs& a, float* out, hipStream_t stream) {
    const int nchunk = plane_chunks(a);
    hipLaunchKernelGGL(warp_feature_kernel, grid(a, nchunk), dim3(256), 0, stream, a, nchunk, out);
    return hipGetLastError();
}

hipError_t launch_sample_coords(const SweepArgs& a, float* ix, float* iy, hipStream_t stream) {
    dim3 grid((a.H * a.W + 255) / 256, a.V, a.B);
    hipLaunchKernelGGL(sample_coords_kernel, grid, dim3(256), 0, stream, a, ix, iy);
    return hipGetLastError();
}

}  // namespace pdepth
