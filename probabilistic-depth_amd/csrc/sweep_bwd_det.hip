// g_src of the plane-sweep backward as an order-independent sum: the same bits from call to call, whatever the order in which
// the adds arrive, however the planes are grouped, whichever other items share the batch.
//
// The contributions are those of the g_src pass of sweep_bwd.hip, bit for bit: the same sample positions and footprints
// (geometry.hpp), the same per-channel chain (val, e, r, w r) in the same order under -ffp-contract=off, the same 16 x 16 tiles,
// per-plane boxes, plane groups staged through an LDS box image, direct adds for a plane whose box alone exceeds the cap, and
// the channel tail.  What differs is the sum (fixed_accum.hpp): a contribution q is scaled by 2^S_b, rounded to an integer and
// added with integer atomics -- ds_add_u64 into the box image, global_atomic_add_x2 into the accumulator of the workspace --,
// and a last pass converts the accumulator into g_src.
//
// Launch sequence, all on the caller's stream, no host synchronisation, no copy to the host:
//   1. hipMemsetAsync of the workspace (the per-item header and the accumulator);
//   2. bounds pre-pass: per item max |g_cost[b]| and, for L2, max |src[b]| and max |ref[b]|, as atomicMax over the bit patterns
//      of |x| (order-independent; a NaN or an infinity wins the maximum);
//   3. scatter (L2 / L1).  Every workgroup derives S_b of its item from the header (item_exponent: a few integer operations):
//      M_b = |gscale| max|g_cost[b]| E_b bounds every contribution, E_b = max|src[b]| + max|ref[b]| for L2 and 1 for L1, and a
//      texel receives at most N = D H W contributions (per view, a (plane, pixel) sample puts at most one tap, of weight <= 1,
//      on it);
//   4. convert: accumulator -> fp32.  An item whose M_b is 0 is 0.  An item whose bound is not finite -- a NaN or an infinity
//      in g_cost[b] (or, L2, in src[b] / ref[b]), or a factor of M_b (or M_b itself) at or above 2^127, where the fp32 chain is
//      no longer certain to stay finite -- is NaN in every element: an integer cannot hold a NaN, and a non-finite gradient
//      anywhere in an item is what an overflow check of the caller looks for.  (The atomic path confines a NaN to the texels it
//      reaches.)  Every other item is untouched by it.
//
// Workspace: 256-byte-rounded header of 16 bytes per item, then one int64 per element of g_src: 8 B V C H W bytes (B = 4, V = 1,
// C = 67: 17.6 MB at 64 x 128, 281 MB at 256 x 512).
//
// LDS: the box image holds 64-bit integers: BCC * BOX_CAP * 8 bytes = 64 KB at BCC = 4, + 64 D bytes of boxes (at most 96 KB at
// D = 512).  BCC = 8 would halve the passes over the sample positions at 128 KB, one workgroup per CU; BCC = 4 measured faster
// (DESIGN.md 6.1.2).
#include <hip/hip_runtime.h>

#include <climits>

#include "capi_util.hpp"
#include "fixed_accum.hpp"
#include "geometry.hpp"
#include "kernels.hpp"

namespace pdepth {

namespace {

using namespace fixed;

constexpr int BT = SWEEP_BWD_TILE;     // tile edge (pixels)
constexpr int BTHREADS = BT * BT;
#ifndef PDEPTH_DET_BCC
#define PDEPTH_DET_BCC 4   // (8: a 128 KB image, one workgroup per CU -- measured slower)
#endif
constexpr int BCC = PDEPTH_DET_BCC;    // channels per pass
constexpr int BOX_CAP = SWEEP_BWD_BOX_CAP;   // texels of the LDS box image: BCC * BOX_CAP * 8 B
constexpr int HDR_WORDS = 4;           // per item: bits of max |g_cost|, max |src|, max |ref|, unused

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

size_t header_bytes(int B) { return ((size_t)B * HDR_WORDS * sizeof(uint32_t) + 255) / 256 * 256; }

// S_b (or EXP_ZERO / EXP_NONFINITE) from the maxima of item b; the scatter and the convert kernel call it on the same words
__device__ __forceinline__ int item_exponent(const uint32_t* __restrict__ h, float gscale, int metric, long long n) {
    const uint32_t gb = h[0], sb = h[1], rb = h[2];
    if (!bits_finite(gb) || (metric == 0 && (!bits_finite(sb) || !bits_finite(rb)))) return EXP_NONFINITE;
    const double limit = 0x1p127;
    const double coef = (double)fabsf(gscale) * (double)__uint_as_float(gb);
    const double e = metric == 0 ? (double)__uint_as_float(sb) + (double)__uint_as_float(rb) : 1.0;
    const double m = coef * e;   // (three fp32 factors: no underflow, no overflow in double)
    if (!(coef < limit && e < limit && m < limit)) return EXP_NONFINITE;
    if (m == 0.0) return EXP_ZERO;
    const float bound = (float)m;
    return det_scale_exponent(bound > 0.0f ? bound : __uint_as_float(1u), n);   // (below the smallest denormal: that one)
}

// grid (blocks, B, 1 | 3): z = 0 g_cost[b] (D H W), 1 src[b] (V views of C H W), 2 ref[b] (C H W)
__global__ __launch_bounds__(256) void sweep_det_bounds_kernel(SweepArgs a, const float* __restrict__ gcost, uint32_t* __restrict__ hdr) {
    const int b = blockIdx.y, which = blockIdx.z;
    const size_t HW = (size_t)a.H * a.W;
    const size_t chw = (size_t)a.C * HW;
    const float* base = which == 0 ? gcost + (size_t)b * a.D * HW : which == 1 ? a.src + (size_t)b * a.src_bstride : a.ref + (size_t)b * a.ref_bstride;
    const size_t n = which == 0 ? (size_t)a.D * HW : chw;
    const int views = which == 1 ? a.V : 1;
    uint32_t m = 0u;
    for (int v = 0; v < views; ++v) {
        const float* p = base + (size_t)v * a.src_vstride;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = max(m, abs_bits(p[i]));
    }
    m = wave_max_bits(m);
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(hdr + HDR_WORDS * b + which, m);
}

template <int METRIC>
__global__ __launch_bounds__(BTHREADS) void sweep_bwd_det_kernel(SweepArgs a, const float* __restrict__ gcost, const uint32_t* __restrict__ hdr,
                                                                 unsigned long long* __restrict__ acc, int tiles_x) {
    extern __shared__ unsigned long long lds[];
    int* box = reinterpret_cast<int*>(lds);   // [4 waves][D][4]: x min, x max, y min, y max of the wave's in-bounds taps of plane k
    unsigned long long* img = lds + 8 * a.D;  // [BCC][box area]
    const int tid = threadIdx.x;
    const int HW = a.H * a.W;
    const int b = blockIdx.y;
    const float gscale = (METRIC == 0 ? 2.0f : 1.0f) / a.sigma;
    const int S = item_exponent(hdr + HDR_WORDS * b, gscale, METRIC, (long long)a.D * HW);
    if (S == EXP_ZERO || S == EXP_NONFINITE) return;   // (the whole workgroup: the convert pass writes this item)
    const int x = (blockIdx.x % tiles_x) * BT + (tid & (BT - 1));
    const int y = (blockIdx.x / tiles_x) * BT + (tid / BT);
    const bool live = x < a.W && y < a.H;
    const int p = live ? y * a.W + x : HW - 1;   // dead lanes shadow the last pixel and add nothing
    // H*W and W as vector registers: the per-channel offsets derived from them stay in vector registers (sweep_bwd.hip)
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
    const float* srcb = a.src + (size_t)b * a.src_bstride;
    asm volatile("v_mov_b64 %0, %1" : "=v"(srcb) : "s"(srcb));   // (vector registers, as hw_v)

    for (int v = 0; v < a.V; ++v) {
        ViewXform xf;
        make_view_xform(a.K + b * 9, a.R + ((size_t)b * a.V + v) * 9, a.t + ((size_t)b * a.V + v) * 3, a.blas_mode, xf);
        float t2a, t2b, t2c;
        ray_term2(xf, r0, r1, r2, t2a, t2b, t2c);
        const float* srcv = srcb + (size_t)v * a.src_vstride;
        unsigned long long* accv = acc + ((size_t)b * a.V + v) * a.C * HW;

        __syncthreads();   // (the previous view's last reads of box[])
        for (int k = 0; k < a.D; ++k) {   // per-plane boxes of the tile's in-bounds taps
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

        {   // this workgroup's BCC channels
            const int cb = blockIdx.z * BCC;
            float rf[BCC];
#pragma unroll
            for (int cc = 0; cc < BCC; ++cc) rf[cc] = refp[min(cb + cc, a.C - 1) * hw_v];
            int k = 0;
            while (k < a.D) {   // groups of planes (workgroup-uniform)
                int ux0 = INT_MAX, ux1 = INT_MIN, uy0 = INT_MAX, uy1 = INT_MIN;
                int k1 = k, bx0 = 0, by0 = 0, bw = 0, area = 0;
                bool staged = false;
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
                    for (int i = tid; i < BCC * area; i += BTHREADS) img[i] = 0ull;
                    __syncthreads();
                } else {
                    k = k1;   // a run of planes without an in-bounds tap: nothing to add
                    continue;
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
                    for (int cc = 0; cc < BCC; ++cc) {   // gather: e and the gradient of the cost term, channel cb + cc
                        const int co = min(cb + cc, a.C - 1) * hw_v;   // (past the last channel: a copy of it, weighted 0)
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
                        rr[cc] = cb + cc < a.C ? r : 0.0f;
                    }
                    if (!m) continue;
                    if (staged) {   // (rows of the image past the last channel are never flushed)
                        unsigned long long* q = img + lo;
#pragma unroll
                        for (int cc = 0; cc < BCC; ++cc) {
                            if (m & 1u) det_add(q, f.nw * rr[cc], S);
                            if (m & 2u) det_add(q + 1, f.ne * rr[cc], S);
                            if (m & 4u) det_add(q + bw, f.sw * rr[cc], S);
                            if (m & 8u) det_add(q + bw + 1, f.se * rr[cc], S);
                            q += area;
                        }
                    } else {
                        unsigned long long* q = accv + (cb * HW + f.y0 * a.W + f.x0);
                        for (int cc = 0; cc < BCC && cb + cc < a.C; ++cc) {
                            if (m & 1u) det_add(q, f.nw * rr[cc], S);
                            if (m & 2u) det_add(q + 1, f.ne * rr[cc], S);
                            if (m & 4u) det_add(q + w_v, f.sw * rr[cc], S);
                            if (m & 8u) det_add(q + w_v + 1, f.se * rr[cc], S);
                            q += hw_v;
                        }
                    }
                }
                if (staged) {   // the group's box image -> the accumulator, one texel per lane, lanes along the box rows
                    __syncthreads();
                    const int nc = min(BCC, a.C - cb);
                    #pragma unroll 1
                    for (int i = tid; i < nc * area; i += BTHREADS) {
                        const int cc = i / area, rr = i - cc * area;
                        const int ry = rr / bw, rx = rr - ry * bw;
                        const unsigned long long val = img[i];
                        if (val != 0ull) atomicAdd(accv + (size_t)(cb + cc) * HW + (by0 + ry) * a.W + (bx0 + rx), val);
                    }
                    __syncthreads();   // (the next group zeroes the image)
                }
                k = k1;
            }
        }
    }
}

// grid (blocks of 256 elements of an item's g_src, B)
__global__ __launch_bounds__(256) void sweep_det_convert_kernel(const uint32_t* __restrict__ hdr, const long long* __restrict__ acc,
                                                                float* __restrict__ gsrc, size_t per_item, float gscale, int metric, long long n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_item) return;
    const int b = blockIdx.y;
    const int S = item_exponent(hdr + HDR_WORDS * b, gscale, metric, n);
    const size_t at = (size_t)b * per_item + i;
    gsrc[at] = S == EXP_ZERO ? 0.0f : S == EXP_NONFINITE ? __uint_as_float(0x7fc00000u) : det_to_float(acc[at], S);
}

size_t lds_bytes(int D) { return (size_t)16 * D * 4 + (size_t)BCC * BOX_CAP * 8; }

}  // namespace

size_t sweep_backward_det_workspace_bytes(int B, int V, int C, int H, int W) {
    return header_bytes(B) + ((size_t)B * V * C * H * W * sizeof(long long) + 255) / 256 * 256;
}

hipError_t launch_sweep_backward_det(const SweepArgs& a, const float* grad_cost, float* grad_src, void* workspace, hipStream_t stream) {
    const size_t HW = (size_t)a.H * a.W;
    const size_t per_item = (size_t)a.V * a.C * HW;
    uint32_t* hdr = static_cast<uint32_t*>(workspace);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + header_bytes(a.B));
    hipError_t e = hipMemsetAsync(workspace, 0, sweep_backward_det_workspace_bytes(a.B, a.V, a.C, a.H, a.W), stream);
    if (e != hipSuccess) return e;
    const size_t per_block = 256 * 16;   // (elements a block of the pre-pass reads at least, up to 512 blocks per item and array)
    const size_t want = ((size_t)(a.D > a.C ? a.D : a.C) * HW + per_block - 1) / per_block;
    const unsigned nblk = (unsigned)(want < 512 ? want : 512);
    hipLaunchKernelGGL(sweep_det_bounds_kernel, dim3(nblk, a.B, a.metric == 0 ? 3 : 1), dim3(256), 0, stream, a, grad_cost, hdr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int tiles_x = (a.W + BT - 1) / BT, tiles_y = (a.H + BT - 1) / BT;
    const size_t lds = lds_bytes(a.D);
    auto go = [&](auto kern) -> hipError_t {
        hipError_t err = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL(kern, dim3(tiles_x * tiles_y, a.B, (a.C + BCC - 1) / BCC), dim3(BTHREADS), lds, stream, a, grad_cost, hdr, acc, tiles_x);
        return hipGetLastError();
    };
    e = a.metric == 0 ? go(sweep_bwd_det_kernel<0>) : go(sweep_bwd_det_kernel<1>);
    if (e != hipSuccess) return e;
    const float gscale = (a.metric == 0 ? 2.0f : 1.0f) / a.sigma;
    hipLaunchKernelGGL(sweep_det_convert_kernel, dim3((unsigned)((per_item + 255) / 256), a.B), dim3(256), 0, stream, hdr,
                       reinterpret_cast<const long long*>(acc), grad_src, per_item, gscale, a.metric, (long long)a.D * (long long)HW);
    return hipGetLastError();
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entries live here, beside their kernels: capi.o does not refer to this object, so a library
// linked from a subset of the objects still links. ------------------------------------------------------------------------------
extern "C" {

int32_t pdepth_det_scale_exponent(float bound, int64_t n) {
    if (n < 1) return pdepth::fixed::EXP_NONFINITE;
    return pdepth::fixed::det_scale_exponent(bound, n);
}

size_t pdepth_sweep_backward_det_workspace_bytes(const pdepth_sweep_desc* desc) {
    if (!desc || !pdepth::capi::dims_positive(desc)) return 0;
    return pdepth::sweep_backward_det_workspace_bytes(desc->B, desc->V, desc->C, desc->H, desc->W);
}

// est_swp_volume_v4 backward with an order-independent grad_src; grad_ref is the gather pass of sweep_bwd.hip (reproducible as it is)
int pdepth_sweep_backward_det_f32(const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* ref, const float* src,
                                  const float* d_candi, const float* grad_cost, float* grad_ref, float* grad_src, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    using namespace pdepth::capi;
    const char* who = "pdepth_sweep_backward_det_f32";
    if (int rc = check_sweep_backward(who, desc, cam, ref, src, d_candi, grad_cost, grad_ref, grad_src)) return rc;
    if (grad_src) {
        const size_t need = pdepth::sweep_backward_det_workspace_bytes(desc->B, desc->V, desc->C, desc->H, desc->W);
        if (int rc = check_workspace(who, workspace, workspace_bytes, need, "; query pdepth_sweep_backward_det_workspace_bytes()")) return rc;
    }
    pdepth::SweepArgs a = make_args(desc, cam, ref, src, d_candi);
    a.fast_div = 0;
    if (grad_ref) {
        if (int rc = launched(pdepth::launch_sweep_backward(a, grad_cost, grad_ref, nullptr, (hipStream_t)stream), who)) return rc;
    }
    if (!grad_src) return PDEPTH_OK;
    return launched(pdepth::launch_sweep_backward_det(a, grad_cost, grad_src, workspace, (hipStream_t)stream), who);
}

}  // extern "C"
