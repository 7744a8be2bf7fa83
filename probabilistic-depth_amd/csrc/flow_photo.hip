// One direction of the photometric term of the unsupervised flow loss (losses/flow_loss.py:13-27, loss_photomatric at its fixed
// max_distance = 1) in one pass each way: the bilinear warp of the other image along the flow, the masked L1 distance, the SSIM
// distance and the ternary census distance of the masked images.  With R = flow_warp(other, flow, pad), x = R m, y = im m and
// N = B H W:
//
//   value = ( w_l1  sum_{b,c,p} |im - R| m                    / (3 N)
//           + w_ssim sum_{b,c,windows} clamp((1 - S(x, y)) / 2, 0, 1) / (3 B (H - 2)(W - 2))
//           + w_ter  sum_{b,p} T(x, y)(p)                       / N )   /   (sum(m) / N)
//   count = sum(m)
//
// S the 3 x 3 valid-window SSIM of ssim.hip, T the census distance of ternary.hip (0 in the border ring).  A weight that is not > 0
// removes its term: it is not multiplied by 0, and the SSIM windows and the census chains of a term that is off are not evaluated.
//
// As a composition this is the HIP warp (a [B,3,H,W] image written), two mask products, an abs, the HIP SSIM and census (two images
// read and one written each) and five means, replayed backwards by autograd.  Here the forward is one launch and the fixed-order
// sum of its partial sums, the backward one launch; nothing per-pixel is written by the forward and nothing of it is kept but
// count.  Only the flow carries a gradient (the images and the mask are data), so the warp's scatter drops out and the whole
// backward is a gather in a fixed order: no atomics, two calls give the same bits.
//
// Every piece of arithmetic is a shared header's: position, taps, value, d_ix / d_iy and the clamp masks (flow_warp_sample.hpp: R
// has the bits of pdepth_flow_warp_f32, and the flow's gradient is formed from g_R exactly as flow_warp.hip's grad_flow pass
// forms it), the window sums, the window chain and its coefficients (ssim_math.hpp: the backward's clamp decision is the
// forward's), the gray value and the pair chain (ternary_math.hpp); and so is every walk over the tile: the window of a pixel, the
// coefficient planes and their gather, the census sum and gather (window_tile.hpp: the bodies ssim.hip and ternary.hip run, here
// with md = 1), the sums (loss_terms_sum.hpp).  What is this file's own: the staging, the L1 term, the channel order.  The
// products with the mask stay products: a NaN behind a zero mask makes the value NaN; an empty mask is 0 / 0 = NaN; a non-finite
// flow has no tap, R = 0 there.
//
// Tile.  A workgroup of 256 threads owns 64 x 8 pixels of one item (blockIdx.z), lanes along W; a thread owns 2 pixels of one
// column.  The height is ternary.hip's, for its reason: with the census on, a pixel costs 8 chains of two square roots and three
// (forward) or four (backward) divisions, all correctly rounded, which outweighs the warp chain and the 27 window taps, so the
// kernels are bound by arithmetic and want many workgroups -- at 8 rows the loss's coarse levels (64 x 208, B = 4) still put 128
// workgroups on the chip, at 16 rows 64.  What the low tile costs is the halo: 66 x 10 chains for 512 pixels forward (1.29 x),
// 68 x 12 backward (1.59 x); its reads come from L2.
//   forward   evaluates the chain for its pixels and a halo of 1 (zeros outside the image), stages x and y, three channels each,
//             and the gray values I(x), I(y) in LDS (21 KiB); the thread that evaluates a pixel of the tile adds its L1 numerator
//             and its m; every thread adds, for each of its 2 pixels that is at least 1 from every border, the three SSIM windows
//             centred on it and its census distance.  Tiles partition pixels and windows: each is counted once.  Four partial
//             sums per workgroup go to the workspace ([4][B tiles]); flow_photo_final_kernel, one workgroup, adds them in a fixed
//             order in double.  No atomics.
//   backward  recomputes the chain with a halo of 2 (the windows that contain a pixel read their own 3 x 3 pixels; the census
//             needs 1) and stages the same six planes and two gray planes (26 KiB).  A thread first takes the census gather of its
//             pixels, g_I(p) = -sum_o (G(p) + G(p+o)) D(p, p+o) with G = g w_ter / (9 N) at the pixels the forward counts and 0
//             elsewhere (census_tile_gather).  Then one channel at a time: G P, G Q, G R of the 66 x 10 windows that touch the tile
//             (8 KiB; zeros for windows that do not exist), a gather per pixel over the up to nine windows that contain it (rows
//             top to bottom, left to right: ssim_tile_coef, ssim_tile_gather), and
//                 g_R,c = -g w_l1 / (3 N) sign0(im_c - R_c) m  +  m sum_windows (G P + G Q x_p + G R y_p) / 9
//                         +  m 255 (0.2989, 0.5870, 0.1140)_c g_I
//             times d_ix(c), d_iy(c) of the pixel's own taps, summed over c in channel order; g = g_value / (count / N).
//             34 KiB of LDS: four workgroups per CU.
//
// Bytes per pixel (H W large): 4 (2 + 1 + 3) read + 48 gathered, nothing written forward, 8 written backward.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "dpv_lanes.hpp"
#include "flow_warp_launch.hpp"
#include "flow_warp_sample.hpp"
#include "kernels.hpp"
#include "loss_terms_math.hpp"
#include "loss_terms_sum.hpp"
#include "window_tile.hpp"

namespace pdepth {

namespace {

constexpr int FP_TH = 8;   // tile height
using FpTile = WindowTile<1, FP_TH>;
constexpr int FP_R = FpTile::R;

struct FpArgs {
    const float* im;      // [B,3,H,W] the image of this side
    const float* other;   // [B,3,H,W] the image that is warped
    const float* flow;    // [B,2,H,W]
    const float* mask;    // [B,1,H,W]
    flow::Geometry g;
    int pad;
};

// the weights (a term is on where its weight is > 0) and the divisors of the three means and of the mask's mean, as floats
struct FpTerms {
    float w_l1, w_ssim, w_ter;
    int on_l1, on_ssim, on_ter;
    float n3, n_w, n;   // 3 N, 3 B (H - 2)(W - 2), N
};

__device__ __forceinline__ flow::Sample fp_sample(const FpArgs& a, int b, int pix, int px, int py) {
    const int HW = a.g.H * a.g.W;
    const float* f = a.flow + (size_t)b * 2 * HW + pix;
    return flow::sample(f[0], f[HW], px, py, a.g, a.pad);
}
__device__ __forceinline__ flow::Texels fp_texels(const FpArgs& a, const flow::Sample& q, int b, int ch) {
    const int W = a.g.W;
    return flow::load(a.other + ((size_t)b * 3 + ch) * a.g.H * W, (long long)q.y0 * W + q.x0, q, W);
}

// what a pixel (inside the image) hands to the three terms
struct FpPixel {
    float x[3], y[3];   // R m, im m
    float d[3];         // im - R
    float m;
};
__device__ __forceinline__ FpPixel fp_pixel(const FpArgs& a, int b, int px, int py) {
    const int W = a.g.W, HW = a.g.H * W, pix = py * W + px;
    const flow::Sample q = fp_sample(a, b, pix, px, py);
    FpPixel p;
    p.m = a.mask[(size_t)b * HW + pix];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float r = flow::value(q, fp_texels(a, q, b, ch));
        const float i = a.im[((size_t)b * 3 + ch) * HW + pix];
        p.d[ch] = i - r;
        p.x[ch] = r * p.m;
        p.y[ch] = i * p.m;
    }
    return p;
}

// rows x cols pixels from (gy0, gx0) of item b into LDS: x, y per channel and, GRAY, their gray values; zeros outside the image.
// onto(p, r, c) sees every pixel that lies inside the image.
template <bool GRAY, class Onto>
__device__ __forceinline__ void fp_stage(const FpArgs& a, int b, int gy0, int gx0, int rows, int cols, float* __restrict__ sx,
                                         float* __restrict__ sy, float* __restrict__ sa, float* __restrict__ sb, Onto onto) {
    const int n = rows * cols;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int r = i / cols, c = i - r * cols;
        const int py = gy0 + r, px = gx0 + c;
        float vx[3] = {0.0f, 0.0f, 0.0f}, vy[3] = {0.0f, 0.0f, 0.0f};
        if (py >= 0 && py < a.g.H && px >= 0 && px < a.g.W) {
            const FpPixel p = fp_pixel(a, b, px, py);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                vx[ch] = p.x[ch];
                vy[ch] = p.y[ch];
            }
            onto(p, r, c);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            sx[ch * n + i] = vx[ch];
            sy[ch * n + i] = vy[ch];
        }
        if (GRAY) {
            sa[i] = ternary_gray255(vx[0], vx[1], vx[2]);
            sb[i] = ternary_gray255(vy[0], vy[1], vy[2]);
        }
    }
}

// a pixel the SSIM centres a window on and the census counts: at least 1 from every border
__device__ __forceinline__ bool fp_inner(int px, int py, int H, int W) { return px >= 1 && px < W - 1 && py >= 1 && py < H - 1; }

__global__ __launch_bounds__(256) void flow_photo_fwd_kernel(FpArgs a, int on_ssim, int on_ter, float* __restrict__ part) {
    constexpr int LW = FpTile::LW, LH = FpTile::LH, LN = LH * LW;
    __shared__ float sx[3 * LN];
    __shared__ float sy[3 * LN];
    __shared__ float sa[LN];
    __shared__ float sb[LN];
    const int H = a.g.H, W = a.g.W;
    const int b = blockIdx.z;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * FP_TH;
    float num = 0.0f, den = 0.0f, dist = 0.0f, tern = 0.0f;
    fp_stage<true>(a, b, y0 - 1, x0 - 1, LH, LW, sx, sy, sa, sb, [&](const FpPixel& p, int r, int c) {
        if (r >= 1 && r <= FP_TH && c >= 1 && c <= TILE_W) {   // a pixel of the tile itself
            num += (fabsf(p.d[0]) * p.m + fabsf(p.d[1]) * p.m) + fabsf(p.d[2]) * p.m;
            den += p.m;
        }
    });
    __syncthreads();
    const auto [tx, ty] = tile_thread();
    const int px = x0 + tx;
#pragma unroll
    for (int k = 0; k < FP_R; ++k) {
        const int ly = ty * FP_R + k;
        const int py = y0 + ly;
        if (!fp_inner(px, py, H, W)) continue;
        if (on_ssim) {   // the window centred on the pixel: its first pixel is (ly, tx) of the stage
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) dist += ssim_tile_dist<1>(sx + ch * LN, sy + ch * LN, ly, tx);
        }
        if (on_ter) tern += census_tile_sum<1>(sa, sb, LW, ly, tx) / 9.0f;   // the patch centred on the pixel
    }
    block_partial({num, den, dist, tern}, part);
}

// the four partial sums of the batch in a fixed order, in double; a term that is off is not read into the value
__global__ __launch_bounds__(256) void flow_photo_final_kernel(const float* __restrict__ part, int nblk, FpTerms t,
                                                               float* __restrict__ value, float* __restrict__ count) {
    float s[4];
    partial_sums(part, (size_t)nblk, 0, nblk, s);
    if (threadIdx.x != 0) return;
    float total = 0.0f;
    if (t.on_l1) total = total + t.w_l1 * (s[0] / t.n3);
    if (t.on_ssim) total = total + t.w_ssim * (s[2] / t.n_w);
    if (t.on_ter) total = total + t.w_ter * (s[3] / t.n);
    value[0] = total / (s[1] / t.n);
    count[0] = s[1];
}

__global__ __launch_bounds__(256) void flow_photo_bwd_kernel(FpArgs a, FpTerms t, const float* __restrict__ count,
                                                             const float* __restrict__ g_value, float* __restrict__ g_flow) {
    constexpr int CW = FpTile::LW, CH = FpTile::LH;               // the windows that touch the tile
    constexpr int IW = FpTile::IW, IH = FpTile::IH, IN = IH * IW;   // the pixels those windows read
    __shared__ float sx[3 * IN];
    __shared__ float sy[3 * IN];
    __shared__ float sa[IN];
    __shared__ float sb[IN];
    __shared__ float cp[CH * CW];
    __shared__ float cq[CH * CW];
    __shared__ float cr[CH * CW];
    const int H = a.g.H, W = a.g.W, HW = H * W;
    const int OH = H - 2, OW = W - 2;
    const int b = blockIdx.z;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * FP_TH;
    const float gq = g_value[0] / (count[0] / t.n);   // d L / d (the sum of the three means)
    const float g_l1 = (gq * t.w_l1) / t.n3;          // d L / d |d_c| m of every pixel
    const float g_dist = (gq * t.w_ssim) / t.n_w;     // d L / d dist of every window
    const float g_ter = ((gq * t.w_ter) / t.n) / 9.0f;   // G of every pixel the census counts
    if (t.on_ter) fp_stage<true>(a, b, y0 - 2, x0 - 2, IH, IW, sx, sy, sa, sb, [](const FpPixel&, int, int) {});
    else fp_stage<false>(a, b, y0 - 2, x0 - 2, IH, IW, sx, sy, sa, sb, [](const FpPixel&, int, int) {});
    __syncthreads();
    const auto [tx, ty] = tile_thread();
    const int px = x0 + tx;
    const int cx = px < W ? px : W - 1;   // (a thread past the image shadows the last pixel and stores nothing)
    flow::Sample q[FP_R];
    float m[FP_R], gi[FP_R], gix[FP_R], giy[FP_R];
#pragma unroll
    for (int k = 0; k < FP_R; ++k) {
        const int ly = ty * FP_R + k;
        const int py = y0 + ly;
        const int cy = py < H ? py : H - 1;
        q[k] = fp_sample(a, b, cy * W + cx, cx, cy);
        m[k] = a.mask[(size_t)b * HW + cy * W + cx];
        gi[k] = 0.0f;
        gix[k] = 0.0f;
        giy[k] = 0.0f;
        if (t.on_ter) {   // G is 0 outside the pixels the forward counts, the gray values 0 outside the image
            const float gp = fp_inner(px, py, H, W) ? g_ter : 0.0f;
            // (the stage has a halo of 2, the patch one of 1: its planes start a row and a column in)
            const CensusGrad a1 = census_tile_gather<1, 3, false>(sa + IW + 1, sb + IW + 1, IW, ly, tx, [&](int, int oy, int ox) {
                return gp + (fp_inner(px + ox, py + oy, H, W) ? g_ter : 0.0f);
            });
            gi[k] = -a1.x * 255.0f;
        }
    }
#pragma unroll 1
    for (int ch = 0; ch < 3; ++ch) {
        const float* xc = sx + ch * IN;
        const float* yc = sy + ch * IN;
        if (t.on_ssim) {
            if (ch > 0) __syncthreads();   // the gather of the channel before is done with the coefficients
            ssim_tile_coef<1, FP_TH, false>(xc, yc, x0, y0, OH, OW, [=](int, int) { return g_dist; }, cp, nullptr, cq, cr);
            __syncthreads();
        }
        const float gray = ch == 0 ? 0.2989f : (ch == 1 ? 0.5870f : 0.1140f);
#pragma unroll
        for (int k = 0; k < FP_R; ++k) {
            const int ly = ty * FP_R + k;
            const int py = y0 + ly;
            const int cy = py < H ? py : H - 1;
            const flow::Texels v = fp_texels(a, q[k], b, ch);
            const float d = a.im[((size_t)b * 3 + ch) * HW + cy * W + cx] - flow::value(q[k], v);
            float gw = 0.0f;
            if (t.on_l1) gw = -(g_l1 * sign0(d)) * m[k];
            if (t.on_ssim) gw += m[k] * ssim_tile_gather<1, false>(xc, yc, cp, nullptr, cq, cr, ly, tx).x;
            if (t.on_ter) gw += m[k] * (gi[k] * gray);
            if (q[k].any()) {   // flow_warp_grad_flow_kernel's sum over the channels
                gix[k] += flow::d_ix(q[k], v) * gw;
                giy[k] += flow::d_iy(q[k], v) * gw;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < FP_R; ++k) {
        const int py = y0 + ty * FP_R + k;
        if (px >= W || py >= H) continue;
        float* gf = g_flow + (size_t)b * 2 * HW + py * W + px;
        gf[0] = ((gix[k] * ((float)W / 2.0f)) * q[k].mx) * 2.0f / (float)(W - 1);
        gf[HW] = ((giy[k] * ((float)H / 2.0f)) * q[k].my) * 2.0f / (float)(H - 1);
    }
}

inline size_t n_blocks(int B, int H, int W) { return (size_t)B * tiles(W, TILE_W) * tiles(H, FP_TH); }

size_t workspace_bytes(int B, int H, int W) { return partial_sums_bytes(4, n_blocks(B, H, W)); }

// a weight as torch forms it from the Python number, and whether its term is on (the reference's `if w > 0`: a NaN is off)
FpTerms terms_of(double w_l1, double w_ssim, double w_ternary, int B, int H, int W) {
    const double n = (double)B * H * W;
    return {(float)w_l1, (float)w_ssim, (float)w_ternary, w_l1 > 0.0, w_ssim > 0.0, w_ternary > 0.0,
            (float)(3.0 * n), (float)(3.0 * B * (H - 2) * (double)(W - 2)), (float)n};
}

}  // namespace

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entries live here, beside their kernels, like those of photo.hip; like cost_volume.o this
// object needs flow_warp.o beside it (flow_warp_launch.hpp: the warp entries' own check of sizes and pad). -------------------------
namespace {

using namespace pdepth;
using namespace pdepth::capi;

// B, H, W, pad and the weights of both entries: what flow_warp takes, a pixel count that is exact in fp32, a tile row per grid y,
// and a window where a term needs one
int check_flow_photo(const char* who, int32_t B, int32_t H, int32_t W, int32_t pad, double w_ssim, double w_ternary) {
    if (int rc = flow::check_flow_warp(who, B, 3, H, W, pad)) return rc;
    if ((w_ssim > 0.0 || w_ternary > 0.0) && (H < 3 || W < 3))
        return fail(PDEPTH_E_ARG, "%s: H=%d, W=%d: the SSIM and census terms need H and W of at least 3", who, H, W);
    if ((long long)B * H * W > (1ll << 24))
        return fail(PDEPTH_E_ARG, "%s: B*H*W must be at most 2^24", who);
    return PDEPTH_OK;
}

}  // namespace

extern "C" {

size_t pdepth_flow_photo_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return (B > 0 && H > 1 && W > 1 && (long long)B * H * W <= (1ll << 24)) ? workspace_bytes(B, H, W) : 0;
}

int pdepth_flow_photo_f32(const float* im, const float* other, const float* flow, const float* mask, int32_t B, int32_t H, int32_t W,
                          int32_t pad, double w_l1, double w_ssim, double w_ternary, float* value, float* count, void* workspace,
                          size_t workspace_bytes_given, void* stream) {
    const char* who = "pdepth_flow_photo_f32";
    if (!im || !other || !flow || !mask) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!value || !count) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_flow_photo(who, B, H, W, pad, w_ssim, w_ternary)) return rc;
    if (int rc = check_workspace(who, workspace, workspace_bytes_given, workspace_bytes(B, H, W),
                                 "; query pdepth_flow_photo_workspace_bytes()"))
        return rc;
    const FpArgs a{im, other, flow, mask, flow::geometry(H, W), pad};
    const FpTerms t = terms_of(w_l1, w_ssim, w_ternary, B, H, W);
    float* part = static_cast<float*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(tiles(W, TILE_W), tiles(H, FP_TH), B);
    hipLaunchKernelGGL(flow_photo_fwd_kernel, grid, dim3(256), 0, s, a, t.on_ssim, t.on_ter, part);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return launched(err, who);
    hipLaunchKernelGGL(flow_photo_final_kernel, dim3(1), dim3(256), 0, s, part, (int)n_blocks(B, H, W), t, value, count);
    return launched(hipGetLastError(), who);
}

int pdepth_flow_photo_backward_f32(const float* im, const float* other, const float* flow, const float* mask, const float* count,
                                   const float* g_value, int32_t B, int32_t H, int32_t W, int32_t pad, double w_l1, double w_ssim,
                                   double w_ternary, float* g_flow, void* stream) {
    const char* who = "pdepth_flow_photo_backward_f32";
    if (!im || !other || !flow || !mask || !count || !g_value || !g_flow) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_flow_photo(who, B, H, W, pad, w_ssim, w_ternary)) return rc;
    if ((const float*)g_flow == flow) return fail(PDEPTH_E_ARG, "%s: the output may not alias the flow", who);
    const FpArgs a{im, other, flow, mask, flow::geometry(H, W), pad};
    const dim3 grid(tiles(W, TILE_W), tiles(H, FP_TH), B);
    hipLaunchKernelGGL(flow_photo_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, terms_of(w_l1, w_ssim, w_ternary, B, H, W),
                       count, g_value, g_flow);
    return launched(hipGetLastError(), who);
}

}  // extern "C"
