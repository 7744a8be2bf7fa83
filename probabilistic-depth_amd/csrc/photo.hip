// The photometric term of self-supervised depth training in one pass each way: the bilinear warp of the source image along the
// target's depth map, the masked L1 distance and the SSIM distance of the masked images, per batch item
// (loss_blocks.rgb_stereo_consistency_loss with ssim_weight = w != 0).  With m = valid & row >= H / 3, x = warped m, y = tgt m,
// n_w = 3 (H - 2 md)(W - 2 md):
//
//   value = (1 - w) sum_c sum(|y_c - x_c| m) / (3 sum(m))  +  w (sum_windows clamp((1 - S(x, y)) / 2, 0, 1) / n_w) / (sum(m) / (H W))
//   count = sum(m)
//
// As a composition this is the HIP warp (a [B,3,H,W] image written), two mask products, an abs, a masked mean, the HIP SSIM
// (two images read, one written) and two more means, replayed backwards by autograd: about twenty launches each way.  Here the
// forward is one launch and the fixed-order sum of its partial sums, the backward one launch; nothing per-pixel is written by the
// forward and nothing of it is kept but count.
//
// Every piece of arithmetic is a shared header's: the sample position, `valid`, the taps, the bilinear value and its derivatives
// (inverse_warp_math.hpp) through the per-pixel chain of the rsc term (loss_terms_math.hpp: rsc_sample, rsc_channel, rsc_pixel,
// rsc_depth_grad), the window sums in ATen's order, the window chain and its coefficients (ssim_math.hpp); and so is every walk
// over the tile: the window of a pixel, the coefficient planes and the gather (window_tile.hpp), the sums (loss_terms_sum.hpp).
// So the mask has the bits of pdepth_inverse_warp_f32's `valid`, a window the bits it has in ssim.hip on the same x and y, and
// the backward's clamp decision is the forward's.  The products with the mask stay products: a NaN behind a zero mask makes its
// item NaN, as in the composition; an empty mask is 0 / 0 = NaN for its item alone.
//
// Tile.  A workgroup of 256 threads owns 64 x 16 pixels of one item (blockIdx.z), lanes along W (window_tile.hpp).
//   forward   evaluates the chain for its pixels and a halo of md on every side ((64 + 2 md)(16 + 2 md) pixels, zeros outside the
//             image) and stages x and y, three channels each, in LDS; the thread that evaluates a pixel of the tile adds its L1
//             numerator and its m, and every thread adds the SSIM distance of the windows centred on its 4 pixels (one column,
//             4 rows) where such a window exists.  Tiles partition the image: every pixel and every window is counted once.
//             Three partial sums per workgroup go to the workspace ([3][B][tiles]); photo_final_kernel, one workgroup per item,
//             adds them in a fixed order in double.  No atomics.
//   backward  one channel at a time (three channels of the (64 + 4 md)(16 + 4 md) staged pixels and their coefficients do not fit
//             the 64 KiB of static LDS at md = 3): stage x_c, y_c; phase 1 writes G P, G Q, G R of the (64 + 2 md)(16 + 2 md)
//             windows that touch the tile (zeros for windows that do not exist; P' is not needed, only x carries a gradient);
//             phase 2 gathers per pixel the (2 md + 1)^2 windows that contain it, rows top to bottom, left to right
//             (ssim_tile_coef, ssim_tile_gather).  Behind the three channels each pixel forms
//                 g_warped_c = -(1 - w) g / (3 count) sign0(d_c) m  +  m sum_{windows containing p} (G P + G Q x_p + G R y_p) / n
//             with G = -1/2 g w / (n_w count / (H W)) on the windows that pass the clamp (inclusive rule), and from it the
//             gradient of the depth exactly as loss_rsc_bwd_kernel does.  A gather in a fixed order: two calls give the same bits.
//
// Bytes per pixel (H W large against md): forward 4 (1 + 3) read + up to 48 gathered, nothing written; backward the same + 4
// written.  The halo is evaluated again by the neighbouring workgroups (its reads come from L2).
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "dpv_lanes.hpp"
#include "inverse_warp_math.hpp"
#include "kernels.hpp"
#include "loss_terms_math.hpp"
#include "loss_terms_sum.hpp"
#include "window_tile.hpp"

namespace pdepth {

namespace {

constexpr int PHOTO_TH = 16;   // tile height

template <int MD>
__global__ __launch_bounds__(256) void photo_fwd_kernel(RscArgs g, float* __restrict__ part) {
    using T = WindowTile<MD, PHOTO_TH>;
    constexpr int LW = T::LW, LH = T::LH;
    __shared__ float sx[3][LH * LW];
    __shared__ float sy[3][LH * LW];
    const int H = g.H, W = g.W;
    const int b = blockIdx.z;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * PHOTO_TH;
    float num = 0.0f, den = 0.0f, dist = 0.0f;
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int r = i / LW, c = i - r * LW;
        const int py = y0 - MD + r, px = x0 - MD + c;
        float vx[3] = {0.0f, 0.0f, 0.0f}, vy[3] = {0.0f, 0.0f, 0.0f};
        if (py >= 0 && py < H && px >= 0 && px < W) {
            const RscPixel p = rsc_pixel<false>(g, b, py * W + px, px, py);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                vx[ch] = p.x[ch];
                vy[ch] = p.y[ch];
            }
            if (r >= MD && r < MD + PHOTO_TH && c >= MD && c < MD + TILE_W) {   // a pixel of the tile itself
                num += (fabsf(p.d[0]) * p.m + fabsf(p.d[1]) * p.m) + fabsf(p.d[2]) * p.m;
                den += p.m;
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            sx[ch][i] = vx[ch];
            sy[ch][i] = vy[ch];
        }
    }
    __syncthreads();
    const auto [tx, ty] = tile_thread();
    const int px = x0 + tx;
#pragma unroll
    for (int k = 0; k < T::R; ++k) {
        const int ly = ty * T::R + k;
        const int py = y0 + ly;
        if (px >= MD && px < W - MD && py >= MD && py < H - MD) {   // the window centred on (px, py): first pixel (ly, tx) of the stage
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) dist += ssim_tile_dist<MD>(sx[ch], sy[ch], ly, tx);
        }
    }
    block_partial({num, den, dist}, part);
}

// the three partial sums of an item in a fixed order, in double (partial_sums):
// value = omw t0 / (3 t1) + w (t2 / n_w) / (t1 / hw), count = t1 (0 / 0 = NaN for an empty mask)
__global__ __launch_bounds__(256) void photo_final_kernel(const float* __restrict__ part, int B, int nblk, float w, float omw, float n_w,
                                                          float hw, float* __restrict__ value, float* __restrict__ count) {
    const int b = blockIdx.x;
    float t[3];
    partial_sums(part, (size_t)B * nblk, (size_t)b * nblk, nblk, t);
    if (threadIdx.x != 0) return;
    const float l1 = t[0] / (3.0f * t[1]);
    const float structural = (t[2] / n_w) / (t[1] / hw);
    value[b] = omw * l1 + w * structural;
    count[b] = t[1];
}

template <int MD>
__global__ __launch_bounds__(256) void photo_bwd_kernel(RscArgs g, const float* __restrict__ count, const float* __restrict__ g_value,
                                                        float w, float omw, float* __restrict__ g_depth) {
    using T = WindowTile<MD, PHOTO_TH>;
    constexpr int IW = T::IW, IH = T::IH;
    __shared__ float sx[IH * IW];
    __shared__ float sy[IH * IW];
    __shared__ float cp[T::LH * T::LW];
    __shared__ float cq[T::LH * T::LW];
    __shared__ float cr[T::LH * T::LW];
    __shared__ float gs[3][PHOTO_TH * TILE_W];   // d L / d x_c of the tile's pixels through the SSIM
    const int H = g.H, W = g.W, HW = H * W;
    const int OH = H - 2 * MD, OW = W - 2 * MD;
    const int b = blockIdx.z;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * PHOTO_TH;
    const float cnt = count[b], gv = g_value[b];
    const float g_dist = (gv * w) / ((float)(3 * OH * OW) * (cnt / (float)HW));   // d L / d dist of every window of the item
    const float g_l1 = (omw * gv) / (3.0f * cnt);                                  // d L / d |d_c| m of every pixel
    const auto [tx, ty] = tile_thread();
    const int px = x0 + tx;
    // (one channel, then one pixel at a time: the unrolled form of the whole holds every load of the gather in registers and spills)
#pragma unroll 1
    for (int ch = 0; ch < 3; ++ch) {
        if (ch > 0) __syncthreads();   // the gather of the channel before is done with the stage
        for (int i = threadIdx.x; i < IH * IW; i += 256) {
            const int r = i / IW, c = i - r * IW;
            const int qy = y0 - 2 * MD + r, qx = x0 - 2 * MD + c;
            float vx = 0.0f, vy = 0.0f;
            if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
                const int pix = qy * W + qx;
                const RscChannel v = rsc_channel<false>(g, rsc_sample(g, b, pix, qx, qy), b, pix, ch);
                vx = v.x;
                vy = v.y;
            }
            sx[i] = vx;
            sy[i] = vy;
        }
        __syncthreads();
        ssim_tile_coef<MD, PHOTO_TH, false>(sx, sy, x0, y0, OH, OW, [=](int, int) { return g_dist; }, cp, nullptr, cq, cr);
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < T::R; ++k) {
            const int ly = ty * T::R + k;
            gs[ch][ly * TILE_W + tx] = ssim_tile_gather<MD, false>(sx, sy, cp, nullptr, cq, cr, ly, tx).x;   // read back by this thread alone
        }
    }
    // the position gradient and the products behind it, as loss_rsc_bwd_kernel forms them
#pragma unroll 1
    for (int k = 0; k < T::R; ++k) {
        const int ly = ty * T::R + k;
        const int py = y0 + ly;
        if (px >= W || py >= H) continue;
        const int pix = py * W + px;
        const RscPixel p = rsc_pixel<true>(g, b, pix, px, py);
        const float gd = g_l1 * p.m;
        float gix = 0.0f, giy = 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float gw = -(gd * sign0(p.d[ch])) * p.m + p.m * gs[ch][ly * TILE_W + tx];
            gix = __builtin_fmaf(gw, p.gx[ch], gix);
            giy = __builtin_fmaf(gw, p.gy[ch], giy);
        }
        g_depth[(size_t)b * HW + pix] = rsc_depth_grad(g, b, px, py, p.q, gix, giy);
    }
}

inline int n_tiles(int H, int W) { return tiles(W, TILE_W) * tiles(H, PHOTO_TH); }

size_t workspace_bytes(int B, int H, int W) { return partial_sums_bytes(3, (size_t)B * n_tiles(H, W)); }

template <int MD>
void launch_fwd(const RscArgs& a, int B, float* part, hipStream_t stream) {
    const dim3 grid(tiles(a.W, TILE_W), tiles(a.H, PHOTO_TH), B);
    hipLaunchKernelGGL(photo_fwd_kernel<MD>, grid, dim3(256), 0, stream, a, part);
}

template <int MD>
void launch_bwd(const RscArgs& a, int B, const float* count, const float* g_value, float w, float omw, float* g_depth,
                hipStream_t stream) {
    const dim3 grid(tiles(a.W, TILE_W), tiles(a.H, PHOTO_TH), B);
    hipLaunchKernelGGL(photo_bwd_kernel<MD>, grid, dim3(256), 0, stream, a, count, g_value, w, omw, g_depth);
}

}  // namespace

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entries live here, beside their kernels, like those of loss_terms.hip and ssim.hip: capi.o does
// not refer to this object, so a library linked from a subset of the objects still links. ------------------------------------------
namespace {

using namespace pdepth;
using namespace pdepth::capi;

// B, H, W, md of both entries: a map of check_map's sizes, md in 1..3, at least one window, a tile row per grid y
int check_photo(const char* who, int32_t B, int32_t H, int32_t W, int32_t md) {
    if (int rc = check_map(who, B, H, W, 1)) return rc;
    if (int rc = check_window(who, "window", H, W, md)) return rc;
    if (H > 65535 * PHOTO_TH) return fail(PDEPTH_E_ARG, "%s: H must be at most %d", who, 65535 * PHOTO_TH);
    return PDEPTH_OK;
}

// the two factors as torch forms them from the Python number: (float)w and (float)(1 - w), the difference taken in double
inline float weight_of(double w) { return (float)w; }
inline float rest_of(double w) { return (float)(1.0 - w); }

}  // namespace

extern "C" {

size_t pdepth_loss_photo_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return (B > 0 && H > 0 && W > 0 && (long long)H * W <= (1ll << 24)) ? workspace_bytes(B, H, W) : 0;
}

// rgb_stereo_consistency_loss with ssim_weight != 0, per item (losses/loss_blocks.py:114-145 with the SSIM of :47-66 mixed in)
int pdepth_loss_photo_f32(const float* src_rgb, const float* tgt_rgb, const float* tgt_depth, const float* Kinv, const float* proj,
                          int32_t B, int32_t H, int32_t W, double ssim_weight, int32_t md, float* value, float* count, void* workspace,
                          size_t workspace_bytes_given, void* stream) {
    const char* who = "pdepth_loss_photo_f32";
    if (!src_rgb || !tgt_rgb || !tgt_depth || !Kinv || !proj) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!value || !count) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_photo(who, B, H, W, md)) return rc;
    if (int rc = check_workspace(who, workspace, workspace_bytes_given, workspace_bytes(B, H, W))) return rc;
    const RscArgs a{src_rgb, tgt_rgb, tgt_depth, Kinv, proj, H, W};
    float* part = static_cast<float*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    for_md(md, [&](auto m) { launch_fwd<decltype(m)::value>(a, B, part, s); });
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return launched(err, who);
    const float n_w = (float)(3 * (H - 2 * md) * (W - 2 * md));
    hipLaunchKernelGGL(photo_final_kernel, dim3(B), dim3(256), 0, s, part, B, n_tiles(H, W), weight_of(ssim_weight), rest_of(ssim_weight),
                       n_w, (float)(H * W), value, count);
    return launched(hipGetLastError(), who);
}

int pdepth_loss_photo_backward_f32(const float* src_rgb, const float* tgt_rgb, const float* tgt_depth, const float* Kinv,
                                   const float* proj, const float* count, const float* g_value, int32_t B, int32_t H, int32_t W,
                                   double ssim_weight, int32_t md, float* g_tgt_depth, void* stream) {
    const char* who = "pdepth_loss_photo_backward_f32";
    if (!src_rgb || !tgt_rgb || !tgt_depth || !Kinv || !proj || !count || !g_value || !g_tgt_depth)
        return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_photo(who, B, H, W, md)) return rc;
    const RscArgs a{src_rgb, tgt_rgb, tgt_depth, Kinv, proj, H, W};
    const float w = weight_of(ssim_weight), omw = rest_of(ssim_weight);
    hipStream_t s = (hipStream_t)stream;
    for_md(md, [&](auto m) { launch_bwd<decltype(m)::value>(a, B, count, g_value, w, omw, g_tgt_depth, s); });
    return launched(hipGetLastError(), who);
}

}  // extern "C"
