// The passes over a 64-wide pixel tile that ssim.hip, photo.hip, ternary.hip and flow_photo.hip share: the tile's geometry, the
// SSIM distance of a window of the tile, the SSIM backward's coefficient planes and its gather, the census sum and the census
// gather.  The arithmetic of a window and of a pair is ssim_math.hpp's and ternary_math.hpp's; this is the one statement of the
// order in which a tile walks them.  A fused kernel has the bits of the op it fuses because both call the same body: every object
// is built with -ffp-contract=off, so the same operations in the same order give the same bits.
//
// A workgroup of 256 threads owns TILE_W x TH pixels (or outputs) of one plane, lanes along W: thread (tx, ty) owns column tx and
// the R = TH / 4 rows ty R ... ty R + R - 1.  What is staged in LDS, row-major:
//   L  the tile with a halo of md: LH x LW.  The forward stage of every op; in the SSIM backward the coefficient planes, one entry
//      per window that touches the tile, a window standing at its first pixel.
//   I  the tile with a halo of 2 md: IH x IW.  The pixels the windows of L read: the SSIM backward's stage.
// How a pixel is staged stays with each kernel (they read different things), and so do the L1 term, the channel order and the
// choice of what is unrolled around these bodies.  No body here asks which kernel called it.
#pragma once
#include <hip/hip_runtime.h>

#include "ssim_math.hpp"
#include "ternary_math.hpp"

namespace pdepth {

namespace {

constexpr int TILE_W = 64;   // tile width: one wave row

// MD the half-width of the window or patch, TH the tile's height
template <int MD, int TH>
struct WindowTile {
    static constexpr int K = 2 * MD + 1;
    static constexpr int R = TH / 4;   // rows of the tile per thread (256 threads = 64 columns x 4 strips)
    static_assert(TILE_W * TH == 256 * R, "a thread per column and strip");
    static constexpr int LW = TILE_W + 2 * MD, LH = TH + 2 * MD;
    static constexpr int IW = TILE_W + 4 * MD, IH = TH + 4 * MD;
};

struct TileThread {
    int tx, ty;   // column, strip
};
__device__ __forceinline__ TileThread tile_thread() { return {(int)(threadIdx.x & 63), (int)(threadIdx.x >> 6)}; }

// tiles of `tile` that cover n
inline int tiles(int n, int tile) { return (n + tile - 1) / tile; }

// ---- SSIM --------------------------------------------------------------------------------------------------------------------------
// the clamped distance of the window whose first pixel is (ly, tx) of the L stage
template <int MD>
__device__ __forceinline__ float ssim_tile_dist(const float* __restrict__ sx, const float* __restrict__ sy, int ly, int tx) {
    constexpr int K = 2 * MD + 1, LW = TILE_W + 2 * MD;
    const SsimWindow w = ssim_window(ssim_sums<K>(sx + ly * LW + tx, sy + ly * LW + tx, LW), (float)(K * K));
    return ssim_clamp01(w.d);
}

// Backward, phase 1.  sx, sy: the I stage of the tile at (x0, y0).  G P, G Q, G R [and, PP, G P'] of the windows of L into cp, cq,
// cr [cpp]; zeros for the windows that do not exist (OH x OW do).  g_of(wy, wx) is the upstream gradient of window (wy, wx).
template <int MD, int TH, bool PP, class Gout>
__device__ __forceinline__ void ssim_tile_coef(const float* __restrict__ sx, const float* __restrict__ sy, int x0, int y0, int OH,
                                               int OW, Gout g_of, float* __restrict__ cp, float* __restrict__ cpp,
                                               float* __restrict__ cq, float* __restrict__ cr) {
    using T = WindowTile<MD, TH>;
    for (int i = threadIdx.x; i < T::LH * T::LW; i += 256) {
        const int wr = i / T::LW, wc = i - wr * T::LW;
        const int wy = y0 - 2 * MD + wr, wx = x0 - 2 * MD + wc;   // the window's first pixel = its index in the output
        SsimCoef c{0.0f, 0.0f, 0.0f, 0.0f};
        if (wy >= 0 && wy < OH && wx >= 0 && wx < OW) {
            const SsimSums t = ssim_sums<T::K>(sx + wr * T::IW + wc, sy + wr * T::IW + wc, T::IW);
            c = ssim_coef(ssim_window(t, (float)(T::K * T::K)), g_of(wy, wx));
        }
        cp[i] = c.p;
        if (PP) cpp[i] = c.pp;
        cq[i] = c.q;
        cr[i] = c.r;
    }
}

struct SsimGrad {
    float x, y;   // d L / d x_p, d L / d y_p (y: 0 unless asked for)
};

// Backward, phase 2.  The gradient of the tile's pixel (ly, tx) through the K^2 windows that contain it: the window dy rows above
// the pixel and dx columns left of it, rows top to bottom, left to right.  YSIDE: the gradient of y beside that of x (needs cpp).
template <int MD, bool YSIDE>
__device__ __forceinline__ SsimGrad ssim_tile_gather(const float* __restrict__ sx, const float* __restrict__ sy,
                                                     const float* __restrict__ cp, const float* __restrict__ cpp,
                                                     const float* __restrict__ cq, const float* __restrict__ cr, int ly, int tx) {
    constexpr int K = 2 * MD + 1, CW = TILE_W + 2 * MD, IW = TILE_W + 4 * MD;
    const float xp = sx[(ly + 2 * MD) * IW + tx + 2 * MD];
    const float yp = sy[(ly + 2 * MD) * IW + tx + 2 * MD];
    float ax = 0.0f, ay = 0.0f;
#pragma unroll
    for (int dy = K - 1; dy >= 0; --dy) {
#pragma unroll
        for (int dx = K - 1; dx >= 0; --dx) {
            const int ci = (ly + 2 * MD - dy) * CW + (tx + 2 * MD - dx);
            const float p = cp[ci], q = cq[ci], r = cr[ci];
            ax += (p + q * xp) + r * yp;
            if (YSIDE) ay += (cpp[ci] + q * yp) + r * xp;
        }
    }
    return {ax / (float)(K * K), ay / (float)(K * K)};
}

// ---- census ------------------------------------------------------------------------------------------------------------------------
// Both take the gray planes sa, sb with rows `stride` floats apart and the pixel (ly, tx) of a tile whose origin lies MD rows and
// columns into them: the patch's first texel is (ly, tx), its centre (ly + MD, tx + MD).  The patch is walked rows top to bottom,
// left to right, without the centre (its own h is exactly 0).

// the sum of h over the patch
template <int MD>
__device__ __forceinline__ float census_tile_sum(const float* __restrict__ sa, const float* __restrict__ sb, int stride, int ly, int tx) {
    constexpr int K = 2 * MD + 1;
    const float c = sa[(ly + MD) * stride + tx + MD], cp = sb[(ly + MD) * stride + tx + MD];
    float sum = 0.0f;
#pragma unroll
    for (int dy = 0; dy < K; ++dy) {
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            if (dy == MD && dx == MD) continue;
            const int q = (ly + dy) * stride + tx + dx;
            sum += ternary_h(sa[q] - c, sb[q] - cp);
        }
    }
    return sum;
}

struct CensusGrad {
    float x, y;   // sum_o w D(p, p+o) of the first image's gray value and of the second's (y: 0 unless asked for)
};

// The backward's gather.  weight(q, oy, ox) is G(p) + G(p + o) of the pair whose neighbour lies at index q of the planes, oy rows
// and ox columns from the centre.  ROWS_AT_ONCE: the rows of the patch that are unrolled together (K: all of them).
template <int MD, int ROWS_AT_ONCE, bool YSIDE, class Weight>
__device__ __forceinline__ CensusGrad census_tile_gather(const float* __restrict__ sa, const float* __restrict__ sb, int stride, int ly,
                                                         int tx, Weight weight) {
    constexpr int K = 2 * MD + 1;
    const float c = sa[(ly + MD) * stride + tx + MD], cp = sb[(ly + MD) * stride + tx + MD];
    float ax = 0.0f, ay = 0.0f;
#pragma unroll ROWS_AT_ONCE
    for (int dy = 0; dy < K; ++dy) {
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            if (dy == MD && dx == MD) continue;
            const int q = (ly + dy) * stride + tx + dx;
            const TernaryDeriv d = ternary_deriv(sa[q] - c, sb[q] - cp);
            const float w = weight(q, dy - MD, dx - MD);
            ax += w * d.dt;
            if (YSIDE) ay += w * d.dtp;
        }
    }
    return {ax, ay};
}

}  // namespace

}  // namespace pdepth
