// Ternary census distance between two images, forward and backward (losses/loss_blocks.py:8-44): the third piece of the
// reference's photometric loss (losses/flow_loss.py:13-27), the one that does not see a brightness difference between two cameras.
//
//   x, y [B,3,H,W] -> out [B,1,H,W],  md = 1 | 2 | 3,  K = 2 md + 1.  With I = (0.2989 r + 0.5870 g + 0.1140 b) 255 of x, I' of y:
//       out(p) = mean over the K^2 offsets o of h(I(p+o) - I(p), I'(p+o) - I'(p))     (ternary_math.hpp)
//   where p is at least md from every border, and 0 in the border ring; no output that is kept reads outside the image.
//
// As a torch composition this is a one-hot conv2d to K^2 channels per image and about ten elementwise passes over [B,K^2,H,W],
// forward and again in autograd.  Here the forward reads the two images and writes one plane; the backward reads the two images
// and g_out and writes one or two images, and keeps nothing from the forward: it recomputes each pair's chain from the inputs.
//
// Tile.  A workgroup of 256 threads owns 64 x 8 pixels of one item and stages I and I' (formed once per staged texel) with a halo of
// md in LDS; the backward stages G = g_out mask / K^2 beside them, with the same halo.  Lanes run along W: a wave reads one LDS row
// at consecutive addresses.  A thread owns 2 pixels of one column.  The work per pixel is K^2 - 1 chains of two square roots and
// three (forward) or five (backward) divisions, all correctly rounded: the kernels are bound by that chain, not by memory, so the
// tile is kept low (8 rows) to put more workgroups on the chip; the halo rows it reads again come from L2.
//   forward   sums h over the offsets, rows top to bottom, left to right (the centre's own h is exactly 0 and is left out).
//   backward  a gather.  The pixel p meets every pair it belongs to twice: as the centre of (p, p+o), and as the neighbour of the
//             centre p-o.  The second pair is the pair (p, p-o) seen from its other end: the same h, the derivatives negated
//             (ternary_math.hpp).  So with D(p, q) = dh/dt of the pair (centre p, neighbour q)
//                 g_I(p) = -sum_o (G(p) + G(p+o)) D(p, p+o)
//             one chain per offset, not two, in a fixed order: no atomics, two calls give the same bits.  Outside the image G is 0,
//             and so is G(p) of any p that has a neighbour there.  g_x = g_I 255 (0.2989, 0.5870, 0.1140), likewise g_y.
// The sum and the gather over a patch are window_tile.hpp's (census_tile_sum, census_tile_gather), where flow_photo.hip takes them
// too; what is this file's own is the staging of the gray planes and of G, and how many rows of a patch the backward unrolls.
//
// Bytes per pixel (H W large against md): forward 12 + 12 read, 4 written; backward 12 + 12 + 4 read, 12 + 12 written.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "kernels.hpp"
#include "window_tile.hpp"

namespace pdepth {

namespace {

constexpr int TERN_TW = 64;   // tile width, for tests/util_ternary.py, which reads this line and the next to lay out its shapes
constexpr int TERN_TH = 8;    // tile height
static_assert(TERN_TW == TILE_W, "the census tile is window_tile.hpp's");

// rows x cols texels of I and I' from (gy0, gx0) of an item into LDS; zeros outside the image (the reference's zero padding)
__device__ __forceinline__ void ternary_stage(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int gy0, int gx0,
                                              int rows, int cols, float* __restrict__ sa, float* __restrict__ sb) {
    const size_t hw = (size_t)H * W;
    for (int i = threadIdx.x; i < rows * cols; i += 256) {
        const int r = i / cols, c = i - r * cols;
        const int gy = gy0 + r, gx = gx0 + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t at = in ? (size_t)gy * W + gx : 0;
        const float a = ternary_gray255(x[at], x[at + hw], x[at + 2 * hw]);
        const float b = ternary_gray255(y[at], y[at + hw], y[at + 2 * hw]);
        sa[i] = in ? a : 0.0f;
        sb[i] = in ? b : 0.0f;
    }
}

template <int MD>
__global__ __launch_bounds__(256) void ternary_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W,
                                                          float* __restrict__ out) {
    using T = WindowTile<MD, TERN_TH>;
    constexpr int K = T::K, LW = T::LW, LH = T::LH;
    __shared__ float sa[LH * LW];
    __shared__ float sb[LH * LW];
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TERN_TH;
    const size_t hw = (size_t)H * W, item = (size_t)blockIdx.z * 3 * hw;
    ternary_stage(x + item, y + item, H, W, y0 - MD, x0 - MD, LH, LW, sa, sb);
    __syncthreads();
    const auto [tx, ty] = tile_thread();
    const int px = x0 + tx;
#pragma unroll
    for (int k = 0; k < T::R; ++k) {
        const int ly = ty * T::R + k;
        const int py = y0 + ly;
        const float sum = census_tile_sum<MD>(sa, sb, LW, ly, tx);
        const bool inner = px >= MD && px < W - MD && py >= MD && py < H - MD;
        if (px < W && py < H) out[(size_t)blockIdx.z * hw + (size_t)py * W + px] = inner ? sum / (float)(K * K) : 0.0f;
    }
}

// g_x or g_y may be nullptr (the same for every thread): that gradient is not stored
template <int MD>
__global__ __launch_bounds__(256, 2) void ternary_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ g_out, int H, int W, float* __restrict__ g_x,
                                                          float* __restrict__ g_y) {
    using T = WindowTile<MD, TERN_TH>;
    constexpr int K = T::K, LW = T::LW, LH = T::LH;
    __shared__ float sa[LH * LW];
    __shared__ float sb[LH * LW];
    __shared__ float sg[LH * LW];
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TERN_TH;
    const size_t hw = (size_t)H * W, item = (size_t)blockIdx.z * 3 * hw;
    ternary_stage(x + item, y + item, H, W, y0 - MD, x0 - MD, LH, LW, sa, sb);
    const float* go = g_out + (size_t)blockIdx.z * hw;
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int r = i / LW, c = i - r * LW;
        const int gy = y0 - MD + r, gx = x0 - MD + c;
        const bool inner = gy >= MD && gy < H - MD && gx >= MD && gx < W - MD;
        const float g = go[inner ? (size_t)gy * W + gx : 0];
        sg[i] = inner ? g / (float)(K * K) : 0.0f;
    }
    __syncthreads();
    const auto [tx, ty] = tile_thread();
    const int px = x0 + tx;
    // one pixel at a time, and at md = 3 one row of offsets at a time: more chains at once do not fit the registers of two waves
    // per SIMD (all 48 of md = 3 spill), and one wave alone issues at half the SIMD's rate
    constexpr int ROWS_AT_ONCE = MD < 3 ? K : 1;
#pragma unroll 1
    for (int k = 0; k < T::R; ++k) {
        const int ly = ty * T::R + k;
        const int py = y0 + ly;
        const float gp = sg[(ly + MD) * LW + tx + MD];
        const CensusGrad a = census_tile_gather<MD, ROWS_AT_ONCE, true>(sa, sb, LW, ly, tx, [&](int q, int, int) { return gp + sg[q]; });
        if (px < W && py < H) {
            const size_t at = item + (size_t)py * W + px;
            const float gi = -a.x * 255.0f, gip = -a.y * 255.0f;
            if (g_x) {
                g_x[at] = gi * 0.2989f;
                g_x[at + hw] = gi * 0.5870f;
                g_x[at + 2 * hw] = gi * 0.1140f;
            }
            if (g_y) {
                g_y[at] = gip * 0.2989f;
                g_y[at + hw] = gip * 0.5870f;
                g_y[at + 2 * hw] = gip * 0.1140f;
            }
        }
    }
}

template <int MD>
void launch_fwd(const float* x, const float* y, int B, int H, int W, float* out, hipStream_t stream) {
    const dim3 grid(tiles(W, TILE_W), tiles(H, TERN_TH), B);
    hipLaunchKernelGGL(ternary_fwd_kernel<MD>, grid, dim3(256), 0, stream, x, y, H, W, out);
}

template <int MD>
void launch_bwd(const float* x, const float* y, const float* g_out, int B, int H, int W, float* g_x, float* g_y, hipStream_t stream) {
    const dim3 grid(tiles(W, TILE_W), tiles(H, TERN_TH), B);
    hipLaunchKernelGGL(ternary_bwd_kernel<MD>, grid, dim3(256), 0, stream, x, y, g_out, H, W, g_x, g_y);
}

}  // namespace

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entries live here, beside their kernels, like those of ssim.hip: capi.o does not refer to this
// object, so a library linked from a subset of the objects still links. ----------------------------------------------------------
namespace {

using namespace pdepth;
using namespace pdepth::capi;

// B, H, W, md of both entries: positive, md in 1..3, at least one interior pixel, an item per grid z, a plane's offsets in an int
int check_ternary(const char* who, int32_t B, int32_t H, int32_t W, int32_t md) {
    if (int rc = check_dims(who, B, 3, H, W)) return rc;
    if (int rc = check_window(who, "patch", H, W, md)) return rc;
    if (B > 65535 || (long long)H * W > (1ll << 30) || H > 65535 * TERN_TH)
        return fail(PDEPTH_E_ARG, "%s: B must be at most 65535, H*W at most 2^30 and H at most %d", who, 65535 * TERN_TH);
    return PDEPTH_OK;
}

}  // namespace

extern "C" {

int pdepth_ternary_f32(const float* x, const float* y, int32_t B, int32_t H, int32_t W, int32_t md, float* out, void* stream) {
    const char* who = "pdepth_ternary_f32";
    if (!x || !y) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!out) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_ternary(who, B, H, W, md)) return rc;
    if ((const float*)out == x || (const float*)out == y) return fail(PDEPTH_E_ARG, "%s: the output may not alias an input", who);
    hipStream_t s = (hipStream_t)stream;
    for_md(md, [&](auto m) { launch_fwd<decltype(m)::value>(x, y, B, H, W, out, s); });
    return launched(hipGetLastError(), who);
}

int pdepth_ternary_backward_f32(const float* x, const float* y, const float* g_out, int32_t B, int32_t H, int32_t W, int32_t md,
                                float* g_x, float* g_y, void* stream) {
    const char* who = "pdepth_ternary_backward_f32";
    if (!x || !y || !g_out) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!g_x && !g_y) return fail(PDEPTH_E_ARG, "%s: no gradient requested", who);
    if (int rc = check_ternary(who, B, H, W, md)) return rc;
    if (g_x == g_y || (const float*)g_x == x || (const float*)g_x == y || (const float*)g_x == g_out || (const float*)g_y == x ||
        (const float*)g_y == y || (const float*)g_y == g_out)
        return fail(PDEPTH_E_ARG, "%s: the outputs may not alias each other or an input", who);
    hipStream_t s = (hipStream_t)stream;
    for_md(md, [&](auto m) { launch_bwd<decltype(m)::value>(x, y, g_out, B, H, W, g_x, g_y, s); });
    return launched(hipGetLastError(), who);
}

}  // extern "C"
