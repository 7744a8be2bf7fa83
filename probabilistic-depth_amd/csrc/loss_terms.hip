// The consistency and smoothness terms of the training loss, one value per batch item, forward and backward.
//
// Replaces depth_stereo_consistency_loss (losses/loss_blocks.py:147-171), rgb_stereo_consistency_loss (:114-145),
// depth_consistency_loss (:173-184), edge_aware_smoothness_loss at one scale (:73-112) and mean_on_mask (:68-71) as BaseLoss
// calls them per item (losses/losses.py:90-194): each a chain of elementwise passes around one inverse_warp
// (utils/inverse_warp.py:174-210) or transform_dmap (:212-253), replayed backwards by autograd.  Here each term is one pass over
// the maps and its backward another; nothing per-pixel is kept between them (the backward recomputes from the inputs).
//
//   dsc    m = valid & lower two thirds & warped > 0;  a = max(tgt m, 1e-3), b = max(warped m, 1e-3);
//          value = sum(clamp(|a - b| / |a + b|, 0, 1) m) / sum(m).  warped = transform_dmap(src)[tap] * src_mask[tap] at the
//          nearest tap of the target pixel's sample position, evaluated in registers.
//   rsc    m = valid & lower two thirds;  value = sum_c sum(|tgt_c m - warped_c m| m) / (3 sum(m)), warped = bilinear taps.
//   dc     p = max(min of the 4x4 block of large, 1e-3), s = max(small, 1e-3), keep = lower two thirds of the small map;
//          value = sum(clamp(|p - s| / |p + s|, 0, 1) keep) / sum(keep).
//   smooth value = mean(|d_y - d_y+1| exp(-mean_c |rgb_y - rgb_y+1|)) + mean(|d_x - d_x+1| exp(-mean_c |rgb_x - rgb_x+1|)).
//
// The sample position, `valid` and the taps are inverse_warp_math.hpp: the bits of pdepth_inverse_warp_f32, so the masks are
// those of the composition.  The products with the mask are kept as products (x * 0, not a skip): a NaN or an infinite depth
// behind a zero mask makes its item NaN exactly where the composition's does, and an item whose mask is empty is 0 / 0 = NaN.
// Clamps propagate a NaN, as torch.clamp does (fmaxf would not).
//
// Bytes per item (h, w: the map the threads walk): dsc forward 4 HW (tgt) + up to 8 HW gathered (src, src_mask at the taps),
// backward the same + 4 HW written (tgt) + 4 HW cleared and scattered (src);  rsc forward 4 HW (1 + 3) + up to 48 HW gathered,
// backward the same + 4 HW written;  dc forward 4 HW + 4 hw, backward the same + 4 HW + 4 hw written;  smooth forward and
// backward 4 HW (1 + 3) with the neighbours from cache, backward + 4 HW written.
//
// Gradient rules are torch's: sign(0) = 0 behind abs, a clamp passes the gradient on min <= x <= max, masks / valid / taps are
// constants.  Only the src_depth gradient of dsc is scattered (dsc_scatter into FloatAtomics: atomicAdd on fp32); every other
// gradient is written by the thread that owns the element: the same bits from call to call.
//
// Pixel reduction (loss_terms_sum.hpp, shared with loss_smooth1.hip): as loss.hip -- a workgroup (256 pixels) writes two partial
// sums into the workspace, a second launch of one workgroup per item adds them in a fixed order in double.  No atomics: two calls
// give the same bits.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "dpv_lanes.hpp"
#include "fixed_accum.hpp"
#include "inverse_warp_math.hpp"
#include "kernels.hpp"
#include "loss_terms_math.hpp"
#include "loss_terms_sum.hpp"

namespace pdepth {

namespace {

// ---- depth stereo consistency (the per-pixel chain: loss_terms_math.hpp) ----------------------------------------------------------
__global__ __launch_bounds__(256) void loss_dsc_kernel(DscArgs g, float* __restrict__ part) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    float num = 0.0f, den = 0.0f;
    if (pix < g.H * g.W) {
        const DscPixel p = dsc_pixel(g, blockIdx.y, pix);
        num = rel_diff(p.a, p.b).diff * p.m;
        den = p.m;
    }
    block_partial({num, den}, part);
}

// g_src (cleared by the launcher) and g_tgt may be nullptr
__global__ __launch_bounds__(256) void loss_dsc_bwd_kernel(DscArgs g, const float* __restrict__ count, const float* __restrict__ g_value,
                                                           float* __restrict__ g_src, float* __restrict__ g_tgt) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = g.H * g.W;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const DscGrad d = dsc_pixel_grad(g, count, g_value, b, pix);
    if (g_tgt) g_tgt[(size_t)b * HW + pix] = d.g_tgt;
    if (g_src) {
        fixed::FloatAtomics sink{g_src};
        dsc_scatter(d, (long long)b * HW, sink);
    }
}

// ---- RGB stereo consistency ----------------------------------------------------------------------------------------------------
// (the per-pixel chain and the camera products of the backward: loss_terms_math.hpp)
__global__ __launch_bounds__(256) void loss_rsc_kernel(RscArgs g, float* __restrict__ part) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    float num = 0.0f, den = 0.0f;
    if (pix < g.H * g.W) {
        const int y = pix / g.W, x = pix - y * g.W;
        const RscPixel p = rsc_pixel<false>(g, blockIdx.y, pix, x, y);
        num = (fabsf(p.d[0]) * p.m + fabsf(p.d[1]) * p.m) + fabsf(p.d[2]) * p.m;
        den = p.m;
    }
    block_partial({num, den}, part);
}

// The position gradient as inverse_warp_bwd_kernel<0> forms it (inverse_warp_math.hpp: the derivatives of the bilinear value,
// point_grad) and the products behind it (the gradient of the camera point, of the depth), per pixel in one thread.
__global__ __launch_bounds__(256) void loss_rsc_bwd_kernel(RscArgs g, const float* __restrict__ count, const float* __restrict__ g_value,
                                                           float* __restrict__ g_depth) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int H = g.H, W = g.W, HW = H * W;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const int y = pix / W, x = pix - y * W;
    const RscPixel p = rsc_pixel<true>(g, b, pix, x, y);
    const WarpSample& q = p.q;
    const float gd = (g_value[b] / (3.0f * count[b])) * p.m;
    float gix = 0.0f, giy = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float gw = -(gd * sign0(p.d[c])) * p.m;   // d |tgt m - warped m| / d warped
        gix = __builtin_fmaf(gw, p.gx[c], gix);
        giy = __builtin_fmaf(gw, p.gy[c], giy);
    }
    g_depth[(size_t)b * HW + pix] = rsc_depth_grad(g, b, x, y, q, gix, giy);
}

// ---- down-sample consistency ---------------------------------------------------------------------------------------------------
// One thread per pixel of the small map [h,w] = [H/4,W/4].  The minimum of the 4x4 block as -max_pool2d(-x, 4) takes it: the
// first element in row-major order wins a tie, a NaN replaces whatever came before.
struct DcPixel {
    float praw, sraw, p, s, keep;
    int arg;   // offset of the minimum inside the large map
};

__device__ __forceinline__ DcPixel dc_pixel(const float* __restrict__ large, const float* __restrict__ small, int b, int lp, int H,
                                            int W, int h, int w) {
    const int ly = lp / w, lx = lp - ly * w;
    const float* blk = large + (size_t)b * H * W + (size_t)(4 * ly) * W + 4 * lx;
    DcPixel p;
    p.arg = (4 * ly) * W + 4 * lx;
    p.praw = blk[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = blk[i * W + j];
            if (v < p.praw || v != v) {
                p.praw = v;
                p.arg = (4 * ly + i) * W + 4 * lx + j;
            }
        }
    }
    p.sraw = small[(size_t)b * h * w + lp];
    p.p = clamp_min(p.praw, FLOOR);
    p.s = clamp_min(p.sraw, FLOOR);
    p.keep = ly >= h / 3 ? 1.0f : 0.0f;
    return p;
}

__global__ __launch_bounds__(256) void loss_dc_kernel(const float* __restrict__ large, const float* __restrict__ small, int H,
                                                      int W, int h, int w, float* __restrict__ part) {
    const int lp = blockIdx.x * 256 + threadIdx.x;
    float num = 0.0f, den = 0.0f;
    if (lp < h * w) {
        const DcPixel p = dc_pixel(large, small, blockIdx.y, lp, H, W, h, w);
        num = rel_diff(p.p, p.s).diff * p.keep;
        den = p.keep;
    }
    block_partial({num, den}, part);
}

// g_large (rows and columns past 4 h, 4 w cleared by the launcher) and g_small may be nullptr
__global__ __launch_bounds__(256) void loss_dc_bwd_kernel(const float* __restrict__ large, const float* __restrict__ small,
                                                          const float* __restrict__ count, const float* __restrict__ g_value, int H,
                                                          int W, int h, int w, float* __restrict__ g_large,
                                                          float* __restrict__ g_small) {
    const int lp = blockIdx.x * 256 + threadIdx.x;
    if (lp >= h * w) return;
    const int b = blockIdx.y;
    const DcPixel p = dc_pixel(large, small, b, lp, H, W, h, w);
    const RelDiff r = rel_diff(p.p, p.s);
    const float gd = (g_value[b] / count[b]) * p.keep;
    float gp, gs;
    rel_diff_grad(r, p.p, p.s, gd, gp, gs);
    if (g_small) g_small[(size_t)b * h * w + lp] = p.sraw >= FLOOR ? gs : 0.0f;
    if (g_large) {
        const int ly = lp / w, lx = lp - ly * w;
        const float gl = p.praw >= FLOOR ? gp : 0.0f;
        float* o = g_large + (size_t)b * H * W;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int off = (4 * ly + i) * W + 4 * lx + j;
                o[off] = off == p.arg ? gl : 0.0f;
            }
        }
    }
}

// ---- edge-aware smoothness (one scale, image and map of one size) ------------------------------------------------------------------
// |d - d'| and exp(-mean_c |rgb - rgb'|) of the pair (pix, pix + step); step = W: the row pair, step = 1: the column pair
__device__ __forceinline__ void smooth_pair(const float* __restrict__ d, const float* __restrict__ rgb, int HW, int pix, int step,
                                            float& diff, float& wgt) {
    diff = d[pix] - d[pix + step];
    const float a0 = fabsf(rgb[pix] - rgb[pix + step]);
    const float a1 = fabsf(rgb[HW + pix] - rgb[HW + pix + step]);
    const float a2 = fabsf(rgb[2 * (size_t)HW + pix] - rgb[2 * (size_t)HW + pix + step]);
    wgt = expf(-(((a0 + a1) + a2) / 3.0f));
}

__global__ __launch_bounds__(256) void loss_smooth_kernel(const float* __restrict__ depth, const float* __restrict__ rgb, int H,
                                                          int W, float* __restrict__ part) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    float rows = 0.0f, cols = 0.0f;
    if (pix < HW) {
        const int b = blockIdx.y;
        const int y = pix / W, x = pix - y * W;
        const float* d = depth + (size_t)b * HW;
        const float* im = rgb + (size_t)b * 3 * HW;
        float diff, wgt;
        if (y < H - 1) {
            smooth_pair(d, im, HW, pix, W, diff, wgt);
            rows = fabsf(diff) * wgt;
        }
        if (x < W - 1) {
            smooth_pair(d, im, HW, pix, 1, diff, wgt);
            cols = fabsf(diff) * wgt;
        }
    }
    block_partial({rows, cols}, part);
}

// each pixel gathers the up-to-four differences it takes part in
__global__ __launch_bounds__(256) void loss_smooth_bwd_kernel(const float* __restrict__ depth, const float* __restrict__ rgb,
                                                              const float* __restrict__ g_value, int H, int W,
                                                              float* __restrict__ g_depth) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const int y = pix / W, x = pix - y * W;
    const float* d = depth + (size_t)b * HW;
    const float* im = rgb + (size_t)b * 3 * HW;
    const float gr = g_value[b] / (float)((H - 1) * W), gc = g_value[b] / (float)(H * (W - 1));
    float out = 0.0f, diff, wgt;
    if (y < H - 1) {
        smooth_pair(d, im, HW, pix, W, diff, wgt);
        out += (gr * wgt) * sign0(diff);
    }
    if (y > 0) {
        smooth_pair(d, im, HW, pix - W, W, diff, wgt);
        out -= (gr * wgt) * sign0(diff);
    }
    if (x < W - 1) {
        smooth_pair(d, im, HW, pix, 1, diff, wgt);
        out += (gc * wgt) * sign0(diff);
    }
    if (x > 0) {
        smooth_pair(d, im, HW, pix - 1, 1, diff, wgt);
        out -= (gc * wgt) * sign0(diff);
    }
    g_depth[(size_t)b * HW + pix] = out;
}

}  // namespace

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entries live here, beside their kernels, like those of loss.hip: capi.o does not refer to this
// object, so a library linked from a subset of the objects still links. -----------------------------------------------------------
namespace {

using namespace pdepth;
using namespace pdepth::capi;

}  // namespace

extern "C" {

size_t pdepth_loss_terms_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return (B > 0 && H > 0 && W > 0 && (long long)H * W <= (1ll << 24)) ? two_sums_workspace_bytes(B, H, W) : 0;
}

// depth_stereo_consistency_loss per item (losses/loss_blocks.py:147-171; transform_dmap utils/inverse_warp.py:212-253)
int pdepth_loss_dsc_f32(const float* src_depth, const float* tgt_depth, const float* src_mask, const float* Kinv, const float* proj,
                        const float* pose_row, int32_t pose_batched, const float* intr, int32_t B, int32_t H, int32_t W, float* value,
                        float* count, void* workspace, size_t workspace_bytes_given, void* stream) {
    const char* who = "pdepth_loss_dsc_f32";
    if (!src_depth || !tgt_depth || !src_mask || !Kinv || !proj || !pose_row || !intr) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!value || !count) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_map(who, B, H, W, 2)) return rc;
    if (int rc = check_workspace(who, workspace, workspace_bytes_given, two_sums_workspace_bytes(B, H, W))) return rc;
    const DscArgs a{src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr, pose_batched ? 4 : 0, H, W};
    const int nblk = n_blocks(H, W);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(loss_dsc_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, a, part);
    return launched(finish<true>(part, B, nblk, 1.0f, 0.0f, value, count, (hipStream_t)stream), who);
}

int pdepth_loss_dsc_backward_f32(const float* src_depth, const float* tgt_depth, const float* src_mask, const float* Kinv,
                                 const float* proj, const float* pose_row, int32_t pose_batched, const float* intr, const float* count,
                                 const float* g_value, int32_t B, int32_t H, int32_t W, float* g_src_depth, float* g_tgt_depth,
                                 void* stream) {
    const char* who = "pdepth_loss_dsc_backward_f32";
    if (!src_depth || !tgt_depth || !src_mask || !Kinv || !proj || !pose_row || !intr || !count || !g_value)
        return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!g_src_depth && !g_tgt_depth) return fail(PDEPTH_E_ARG, "%s: no gradient requested", who);
    if (int rc = check_map(who, B, H, W, 2)) return rc;
    if (g_src_depth) {
        hipError_t e = pdepth::launch_zero(g_src_depth, (size_t)B * H * W * sizeof(float), (hipStream_t)stream);
        if (e != hipSuccess) return launched(e, who);
    }
    const DscArgs a{src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr, pose_batched ? 4 : 0, H, W};
    hipLaunchKernelGGL(loss_dsc_bwd_kernel, dim3(n_blocks(H, W), B), dim3(256), 0, (hipStream_t)stream, a, count, g_value, g_src_depth,
                       g_tgt_depth);
    return launched(hipGetLastError(), who);
}

// rgb_stereo_consistency_loss per item (losses/loss_blocks.py:114-145)
int pdepth_loss_rsc_f32(const float* src_rgb, const float* tgt_rgb, const float* tgt_depth, const float* Kinv, const float* proj,
                        int32_t B, int32_t H, int32_t W, float* value, float* count, void* workspace, size_t workspace_bytes_given,
                        void* stream) {
    const char* who = "pdepth_loss_rsc_f32";
    if (!src_rgb || !tgt_rgb || !tgt_depth || !Kinv || !proj) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!value || !count) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_map(who, B, H, W, 2)) return rc;
    if (int rc = check_workspace(who, workspace, workspace_bytes_given, two_sums_workspace_bytes(B, H, W))) return rc;
    const RscArgs a{src_rgb, tgt_rgb, tgt_depth, Kinv, proj, H, W};
    const int nblk = n_blocks(H, W);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(loss_rsc_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, a, part);
    return launched(finish<true>(part, B, nblk, 3.0f, 0.0f, value, count, (hipStream_t)stream), who);
}

int pdepth_loss_rsc_backward_f32(const float* src_rgb, const float* tgt_rgb, const float* tgt_depth, const float* Kinv,
                                 const float* proj, const float* count, const float* g_value, int32_t B, int32_t H, int32_t W,
                                 float* g_tgt_depth, void* stream) {
    const char* who = "pdepth_loss_rsc_backward_f32";
    if (!src_rgb || !tgt_rgb || !tgt_depth || !Kinv || !proj || !count || !g_value || !g_tgt_depth)
        return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_map(who, B, H, W, 2)) return rc;
    const RscArgs a{src_rgb, tgt_rgb, tgt_depth, Kinv, proj, H, W};
    hipLaunchKernelGGL(loss_rsc_bwd_kernel, dim3(n_blocks(H, W), B), dim3(256), 0, (hipStream_t)stream, a, count, g_value, g_tgt_depth);
    return launched(hipGetLastError(), who);
}

// depth_consistency_loss per item (losses/loss_blocks.py:173-184; minpool utils/img_utils.py:87-95): H, W of the large map
int pdepth_loss_dc_f32(const float* large, const float* small, int32_t B, int32_t H, int32_t W, float* value, float* count,
                       void* workspace, size_t workspace_bytes_given, void* stream) {
    const char* who = "pdepth_loss_dc_f32";
    if (!large || !small) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!value || !count) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_map(who, B, H, W, 4)) return rc;
    const int h = H / 4, w = W / 4;
    if (int rc = check_workspace(who, workspace, workspace_bytes_given, two_sums_workspace_bytes(B, h, w))) return rc;
    const int nblk = n_blocks(h, w);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(loss_dc_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, large, small, H, W, h, w, part);
    return launched(finish<true>(part, B, nblk, 1.0f, 0.0f, value, count, (hipStream_t)stream), who);
}

int pdepth_loss_dc_backward_f32(const float* large, const float* small, const float* count, const float* g_value, int32_t B,
                                int32_t H, int32_t W, float* g_large, float* g_small, void* stream) {
    const char* who = "pdepth_loss_dc_backward_f32";
    if (!large || !small || !count || !g_value) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!g_large && !g_small) return fail(PDEPTH_E_ARG, "%s: no gradient requested", who);
    if (int rc = check_map(who, B, H, W, 4)) return rc;
    const int h = H / 4, w = W / 4;
    if (g_large && (H % 4 != 0 || W % 4 != 0)) {   // the rows and columns max_pool2d drops
        hipError_t e = pdepth::launch_zero(g_large, (size_t)B * H * W * sizeof(float), (hipStream_t)stream);
        if (e != hipSuccess) return launched(e, who);
    }
    hipLaunchKernelGGL(loss_dc_bwd_kernel, dim3(n_blocks(h, w), B), dim3(256), 0, (hipStream_t)stream, large, small, count, g_value, H,
                       W, h, w, g_large, g_small);
    return launched(hipGetLastError(), who);
}

// edge_aware_smoothness_loss at one scale, per item (losses/loss_blocks.py:73-112): depth [B,H,W], rgb [B,3,H,W]
int pdepth_loss_smooth_f32(const float* depth, const float* rgb, int32_t B, int32_t H, int32_t W, float* value, void* workspace,
                           size_t workspace_bytes_given, void* stream) {
    const char* who = "pdepth_loss_smooth_f32";
    if (!depth || !rgb) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!value) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_map(who, B, H, W, 2)) return rc;
    if (int rc = check_workspace(who, workspace, workspace_bytes_given, two_sums_workspace_bytes(B, H, W))) return rc;
    const int nblk = n_blocks(H, W);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(loss_smooth_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, depth, rgb, H, W, part);
    return launched(finish<false>(part, B, nblk, (float)((H - 1) * W), (float)(H * (W - 1)), value, nullptr, (hipStream_t)stream), who);
}

int pdepth_loss_smooth_backward_f32(const float* depth, const float* rgb, const float* g_value, int32_t B, int32_t H, int32_t W,
                                    float* g_depth, void* stream) {
    const char* who = "pdepth_loss_smooth_backward_f32";
    if (!depth || !rgb || !g_value || !g_depth) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_map(who, B, H, W, 2)) return rc;
    hipLaunchKernelGGL(loss_smooth_bwd_kernel, dim3(n_blocks(H, W), B), dim3(256), 0, (hipStream_t)stream, depth, rgb, g_value, H, W,
                       g_depth);
    return launched(hipGetLastError(), who);
}

}  // extern "C"
