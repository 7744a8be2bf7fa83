// SSIM distance between two images, forward and backward (losses/loss_blocks.py:47-66): the photometric term the reference's flow
// loss mixes into its L1 (losses/flow_loss.py:13-27) and carries, commented out, in its RGB consistency term (loss_blocks.py:128-129).
//
//   x, y [B,C,H,W] -> dist [B,C,H-2md,W-2md],  md = 1 | 2 | 3,  one value per (2 md + 1)^2 window (valid windows only, no padding).
//
// As a torch composition this is five average-pool passes and about fifteen elementwise ones, forward and again in autograd.  Here
// the forward reads the two planes and writes one; the backward reads the two planes and g_out and writes one or two planes, and
// keeps nothing from the forward: it recomputes the chain of each window (ssim_math.hpp) from the inputs.
//
// Tile.  A workgroup of 256 threads owns 64 x 16 elements of one plane (forward: outputs; backward: pixels) and stages x and y with
// their halo in LDS: 2 md more rows and columns for the forward, 4 md for the backward (the windows that touch the tile's pixels
// reach 2 md beyond it on every side).  Lanes run along W: a wave reads one LDS row at consecutive addresses.
//   forward   a thread owns 4 outputs of one column and sums each window from LDS in the reference's order (ssim_math.hpp: a running
//             sum over the taps keeps the reference's bits; sharing row sums between the 4 windows would not);
//   backward  phase 1 writes G P, G P', G Q, G R of the (64 + 2 md) x (16 + 2 md) windows that touch the tile into LDS (zeros for the
//             windows that do not exist); phase 2 gathers, per pixel, the (2 md + 1)^2 windows that contain it, rows top to bottom,
//             left to right.  A gather in a fixed order, no atomics: two calls give the same bits.
// The tile's geometry, the window of a tile pixel and both phases of the backward are window_tile.hpp's, where photo.hip and
// flow_photo.hip take them too; what is this file's own is the staging of two planes and the upstream gradient per window.
// The halo is read again by the neighbouring workgroups (from L2): (64 + 2 md)(16 + 2 md) / 1024 = 1.16 / 1.33 / 1.50 times the
// plane for the forward, 1.33 / 1.69 / 2.09 times for the backward.
//
// Bytes per element (H W large against md): forward 4 + 4 read, 4 written = 12; backward 4 + 4 + 4 read, 4 + 4 written = 20 with
// both gradients, 16 with one.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "kernels.hpp"
#include "window_tile.hpp"

namespace pdepth {

namespace {

constexpr int SSIM_TH = 16;   // tile height

// rows x cols floats of x and y from (gy0, gx0) of a plane into LDS; zeros outside the plane
__device__ __forceinline__ void ssim_stage(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int gy0, int gx0,
                                           int rows, int cols, float* __restrict__ sx, float* __restrict__ sy) {
    for (int i = threadIdx.x; i < rows * cols; i += 256) {
        const int r = i / cols, c = i - r * cols;
        const int gy = gy0 + r, gx = gx0 + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t at = in ? (size_t)gy * W + gx : 0;
        const float vx = x[at], vy = y[at];
        sx[i] = in ? vx : 0.0f;
        sy[i] = in ? vy : 0.0f;
    }
}

template <int MD>
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W,
                                                       float* __restrict__ out) {
    using T = WindowTile<MD, SSIM_TH>;
    __shared__ float sx[T::LH * T::LW];
    __shared__ float sy[T::LH * T::LW];
    const int OH = H - 2 * MD, OW = W - 2 * MD;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * SSIM_TH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    ssim_stage(x + plane, y + plane, H, W, y0, x0, T::LH, T::LW, sx, sy);
    __syncthreads();
    const auto [tx, ty] = tile_thread();
    const int ox = x0 + tx;
    float* o = out + (size_t)blockIdx.z * OH * OW;
#pragma unroll
    for (int k = 0; k < T::R; ++k) {
        const int ly = ty * T::R + k;
        const float d = ssim_tile_dist<MD>(sx, sy, ly, tx);
        const int oy = y0 + ly;
        if (ox < OW && oy < OH) o[(size_t)oy * OW + ox] = d;
    }
}

// g_x or g_y may be nullptr (the same for every thread): that gradient is not stored
template <int MD>
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ g_out, int H, int W, float* __restrict__ g_x,
                                                       float* __restrict__ g_y) {
    using T = WindowTile<MD, SSIM_TH>;
    __shared__ float sx[T::IH * T::IW];
    __shared__ float sy[T::IH * T::IW];
    __shared__ float cp[T::LH * T::LW];
    __shared__ float cpp[T::LH * T::LW];
    __shared__ float cq[T::LH * T::LW];
    __shared__ float cr[T::LH * T::LW];
    const int OH = H - 2 * MD, OW = W - 2 * MD;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * SSIM_TH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    ssim_stage(x + plane, y + plane, H, W, y0 - 2 * MD, x0 - 2 * MD, T::IH, T::IW, sx, sy);
    __syncthreads();
    const float* go = g_out + (size_t)blockIdx.z * OH * OW;
    ssim_tile_coef<MD, SSIM_TH, true>(sx, sy, x0, y0, OH, OW, [=](int wy, int wx) { return go[(size_t)wy * OW + wx]; }, cp, cpp, cq, cr);
    __syncthreads();
    const auto [tx, ty] = tile_thread();
    const int px = x0 + tx;
#pragma unroll
    for (int k = 0; k < T::R; ++k) {
        const int ly = ty * T::R + k;
        const int py = y0 + ly;
        const SsimGrad g = ssim_tile_gather<MD, true>(sx, sy, cp, cpp, cq, cr, ly, tx);
        if (px < W && py < H) {
            const size_t at = plane + (size_t)py * W + px;
            if (g_x) g_x[at] = g.x;
            if (g_y) g_y[at] = g.y;
        }
    }
}

template <int MD>
void launch_fwd(const float* x, const float* y, int BC, int H, int W, float* out, hipStream_t stream) {
    const dim3 grid(tiles(W - 2 * MD, TILE_W), tiles(H - 2 * MD, SSIM_TH), BC);
    hipLaunchKernelGGL(ssim_fwd_kernel<MD>, grid, dim3(256), 0, stream, x, y, H, W, out);
}

template <int MD>
void launch_bwd(const float* x, const float* y, const float* g_out, int BC, int H, int W, float* g_x, float* g_y, hipStream_t stream) {
    const dim3 grid(tiles(W, TILE_W), tiles(H, SSIM_TH), BC);
    hipLaunchKernelGGL(ssim_bwd_kernel<MD>, grid, dim3(256), 0, stream, x, y, g_out, H, W, g_x, g_y);
}

}  // namespace

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entries live here, beside their kernels, like those of loss_terms.hip: capi.o does not refer to
// this object, so a library linked from a subset of the objects still links. --------------------------------------------------------
namespace {

using namespace pdepth;
using namespace pdepth::capi;

// B, C, H, W, md of both entries: positive, md in 1..3, at least one window, one plane per grid z, a plane's offsets in an int
int check_ssim(const char* who, int32_t B, int32_t C, int32_t H, int32_t W, int32_t md) {
    if (int rc = check_dims(who, B, C, H, W)) return rc;
    if (int rc = check_window(who, "window", H, W, md)) return rc;
    if ((long long)B * C > 65535 || (long long)H * W > (1ll << 30) || H > 65535 * SSIM_TH)
        return fail(PDEPTH_E_ARG, "%s: B*C must be at most 65535, H*W at most 2^30 and H at most %d", who, 65535 * SSIM_TH);
    return PDEPTH_OK;
}

}  // namespace

extern "C" {

int pdepth_ssim_f32(const float* x, const float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t md, float* out, void* stream) {
    const char* who = "pdepth_ssim_f32";
    if (!x || !y) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!out) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_ssim(who, B, C, H, W, md)) return rc;
    hipStream_t s = (hipStream_t)stream;
    for_md(md, [&](auto m) { launch_fwd<decltype(m)::value>(x, y, B * C, H, W, out, s); });
    return launched(hipGetLastError(), who);
}

int pdepth_ssim_backward_f32(const float* x, const float* y, const float* g_out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t md,
                             float* g_x, float* g_y, void* stream) {
    const char* who = "pdepth_ssim_backward_f32";
    if (!x || !y || !g_out) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!g_x && !g_y) return fail(PDEPTH_E_ARG, "%s: no gradient requested", who);
    if (int rc = check_ssim(who, B, C, H, W, md)) return rc;
    if (g_x == g_y || (const float*)g_x == x || (const float*)g_x == y || (const float*)g_x == g_out || (const float*)g_y == x ||
        (const float*)g_y == y || (const float*)g_y == g_out)
        return fail(PDEPTH_E_ARG, "%s: the outputs may not alias each other or an input", who);
    hipStream_t s = (hipStream_t)stream;
    for_md(md, [&](auto m) { launch_bwd<decltype(m)::value>(x, y, g_out, B * C, H, W, g_x, g_y, s); });
    return launched(hipGetLastError(), who);
}

}  // extern "C"
