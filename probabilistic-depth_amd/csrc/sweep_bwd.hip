// Backward of the plane sweep with respect to the feature maps: g_cost [B,D,H,W] -> g_ref [B,C,H,W], g_src [B,V,C,H,W].
//
// Differentiates est_swp_volume_v4 (warping/homography.py:98-135: grid_sample bilinear / zeros / align_corners=False,
// :170-198, then img_dis_L2_pard / img_dis_L1_pard :80-86 and the division by sigma).  With w_v the bilinear warp of view v
// into plane k at pixel p and e = w_v(src_v)[c] - ref[c]:
//     L2: g_ref[c,p] = -(2/sigma) sum_v sum_k g[k,p] e,   tap t of (v,k,p) receives (2/sigma) g[k,p] w_t e in g_src[v,c,t]
//     L1: the same with 2e replaced by sign(e), sign(0) = 0 (torch.abs backward)
// Taps outside the image receive nothing (ATen's grid_sampler_2d backward).  Sample positions and bilinear weights come from
// the helpers the gather kernel uses (geometry.hpp plane_sample_pos / make_footprint, sweep_direct.hip), evaluated in plain
// fp32 on the NCHW features: no distance form, no fp16 pairs, no routing.
//
// One workgroup owns a 16 x 16 tile of reference pixels of one batch item and BCC channels (grid z), every view and every
// plane.  The two outputs are two instantiations, launched one after the other when both are requested
// (one kernel for both did not fit the scalar register file):
//   * g_ref is a per-pixel gather kept in registers and written by the thread that owns the pixel (view after view, read back
//     and added in view order): no atomics, bitwise reproducible from call to call;
//   * g_src is a scatter.  Per view the workgroup first reduces, plane by plane, the bounding box of the in-bounds taps of its
//     tile (LDS).  Consecutive planes are grouped while the union of their boxes fits BOX_CAP texels; a group's taps are summed
//     in an LDS image of the box (ds_add_f32), which is then added to g_src with global_atomic_add_f32, row-contiguous (the
//     lanes of a wave cover consecutive texels of a box row).  A plane whose box alone does not fit (degenerate geometry,
//     near planes of wide baselines) adds its taps to g_src directly: correct, slower.  The launcher zeroes g_src on the
//     stream first.  The sums of g_src depend on the order in which the adds arrive: results may differ in the last bits
//     from call to call.
#include <hip/hip_runtime.h>

#include <climits>

#include "geometry.hpp"
#include "kernels.hpp"

namespace pdepth {

namespace {

constexpr int BT = 16;            // tile edge (pixels)
constexpr int BTHREADS = BT * BT;
constexpr int BCC = 8;            // channels per pass
constexpr int BOX_CAP = 2048;     // texels of the LDS box image: BCC * BOX_CAP * 4 B = 64 KB
static_assert(BT == SWEEP_BWD_TILE && BOX_CAP == SWEEP_BWD_BOX_CAP, "sweep_bwd_det.hip forms the same plane groups");

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

template <int METRIC, bool GREF, bool GSRC>   // GREF / GSRC: the outputs requested (gref / gsrc are not null)
__global__ __launch_bounds__(BTHREADS) void sweep_bwd_kernel(SweepArgs a, const float* __restrict__ gcost,
                                                             float* __restrict__ gref, float* __restrict__ gsrc, int tiles_x) {
    extern __shared__ float lds[];
    int* box = reinterpret_cast<int*>(lds);   // [4 waves][D][4]: x min, x max, y min, y max of the wave's in-bounds taps of plane k
    float* img = lds + 16 * a.D;              // [BCC][box area]
    const int tid = threadIdx.x;
    const int HW = a.H * a.W;
    const int b = blockIdx.y;
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
        float* gsrcv = gsrc + ((size_t)b * a.V + v) * a.C * HW;   // (unused without GSRC)

        if (GSRC) {   // per-plane boxes of the tile's in-bounds taps
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
            float rf[BCC], gr[BCC];
#pragma unroll
            for (int cc = 0; cc < BCC; ++cc) {
                rf[cc] = refp[min(c0 + cc, a.C - 1) * hw_v];
                gr[cc] = 0.0f;
            }
            int k = 0;
            while (k < a.D) {   // groups of planes (workgroup-uniform)
                int k1 = a.D, bx0 = 0, by0 = 0, bw = 0, area = 0;
                bool staged = false;
                if (GSRC) {
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
                        for (int i = tid; i < BCC * area; i += BTHREADS) img[i] = 0.0f;
                        __syncthreads();
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
                        gr[cc] = gr[cc] - rr[cc];
                    }
                    if (staged) {   // (rows of the image past the last channel are never flushed)
                        if (m) {
                            float* q = img + lo;
#pragma unroll
                            for (int cc = 0; cc < BCC; ++cc) {
                                if (m & 1u) atomicAdd(q, f.nw * rr[cc]);
                                if (m & 2u) atomicAdd(q + 1, f.ne * rr[cc]);
                                if (m & 4u) atomicAdd(q + bw, f.sw * rr[cc]);
                                if (m & 8u) atomicAdd(q + bw + 1, f.se * rr[cc]);
                                q += area;
                            }
                        }
                    } else if (GSRC && m) {
                        float* q = gsrcv + (c0 * HW + f.y0 * a.W + f.x0);
                        for (int cc = 0; cc < BCC && c0 + cc < a.C; ++cc) {
                            if (m & 1u) atomicAdd(q, f.nw * rr[cc]);
                            if (m & 2u) atomicAdd(q + 1, f.ne * rr[cc]);
                            if (m & 4u) atomicAdd(q + w_v, f.sw * rr[cc]);
                            if (m & 8u) atomicAdd(q + w_v + 1, f.se * rr[cc]);
                            q += hw_v;
                        }
                    }
                }
                if (staged) {   // the group's box image -> g_src, one texel per lane, lanes along the box rows
                    __syncthreads();
                    const int nc = min(BCC, a.C - c0);
                    #pragma unroll 1
                    for (int i = tid; i < nc * area; i += BTHREADS) {
                        const int cc = i / area, rr = i - cc * area;
                        const int ry = rr / bw, rx = rr - ry * bw;
                        const float val = img[i];
                        if (val != 0.0f) atomicAdd(gsrcv + (size_t)(c0 + cc) * HW + (by0 + ry) * a.W + (bx0 + rx), val);
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
                        *o = v == 0 ? gr[cc] : *o + gr[cc];   // views in order: reproducible
                    }
                }
            }
        }
    }
}

}  // namespace

static size_t sweep_bwd_lds_bytes(int D) { return (size_t)16 * D * 4 + (size_t)BCC * BOX_CAP * 4; }

hipError_t launch_sweep_backward(const SweepArgs& a, const float* grad_cost, float* grad_ref, float* grad_src, hipStream_t stream) {
    const size_t HW = (size_t)a.H * a.W;
    if (grad_src) {
        hipError_t e = hipMemsetAsync(grad_src, 0, (size_t)a.B * a.V * a.C * HW * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    const int tiles_x = (a.W + BT - 1) / BT, tiles_y = (a.H + BT - 1) / BT;
    auto go = [&](auto kern, size_t lds) -> hipError_t {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(tiles_x * tiles_y, a.B, (a.C + BCC - 1) / BCC), dim3(BTHREADS), lds, stream, a, grad_cost, grad_ref,
                           grad_src, tiles_x);
        return hipGetLastError();
    };
    // both outputs: two launches (the gather pass is cheap beside the scatter; one kernel for both did not fit the scalar file)
    hipError_t e = hipSuccess;
    if (grad_ref) e = a.metric == 0 ? go(sweep_bwd_kernel<0, true, false>, 0) : go(sweep_bwd_kernel<1, true, false>, 0);
    const size_t lds = sweep_bwd_lds_bytes(a.D);
    if (e == hipSuccess && grad_src)
        e = a.metric == 0 ? go(sweep_bwd_kernel<0, false, true>, lds) : go(sweep_bwd_kernel<1, false, true>, lds);
    return e;
}

}  // namespace pdepth
