// The per-sample chain of flow_warp (utils/warp_utils.py:82-89 over F.grid_sample, bilinear, align_corners=False), shared by the
// forward, the two gradients, the deterministic scatter and the forward-backward check of flow_warp.hip: positions, taps and
// weights are formed here and nowhere else, so the backward scatters through the forward's taps bit for bit.
//
// The chain of pixel (row y, column x) with flow (fx, fy).  The position is formed in double from the fp32 flow and never
// rounded to fp32 -- the reference's own fp32 chain, 2 v / (W - 1) - 1 and back through ((g + 1) W - 1) / 2, rounds the
// normalised coordinate near 1 and is W / 2 eps32 off everywhere in the image (2.5e-5 px at W = 832); a handful of double
// operations per pixel, not per channel, cost nothing next to the gathers:
//     vx = double(x) + double(fx)   (exact)          ix = vx rx - 0.5,   rx = double(W) / double(W - 1)   (Geometry, from the host)
// and likewise iy: the reference's mixed normalisation, ix = vx W / (W - 1) - 0.5.  A position that is not finite here has no tap,
// in both paddings.  Border padding then clamps ix to [0, W - 1] and iy to [0, H - 1].  x0 = floor(ix), x1 = x0 + 1; the fractions
// w = ix - x0, e = x1 - ix, n = iy - y0, s = y1 - iy are rounded to fp32 once; from there fp32, one rounding per operation, no fma
// (-ffp-contract=off): the weights nw = e s, ne = w s, sw = e n, se = w n; each tap is tested for bounds on its own (border
// padding at ix = W - 1: the x1 column is outside and its weight is 0).
//     value = ((v_nw nw + v_ne ne) + v_sw sw) + v_se se          (an out-of-bounds tap reads 0)
//     d value / d ix = (v_ne - v_nw) s + (v_se - v_sw) n,        d value / d iy = (v_sw - v_nw) e + (v_se - v_ne) w
//     d ix / d fx = (W / 2) (2 / (W - 1)) mx,   mx = 0 where border padding clamped a position strictly outside [0, W - 1], else 1
#pragma once
#include <hip/hip_runtime.h>

namespace pdepth {
namespace flow {

enum { PAD_BORDER = 0, PAD_ZEROS = 1 };

// what is fixed for a launch
struct Geometry {
    int H, W;
    double rx, ry;   // W / (W - 1), H / (H - 1)
};
inline Geometry geometry(int H, int W) { return {H, W, (double)W / (double)(W - 1), (double)H / (double)(H - 1)}; }

struct Sample {
    float nw, ne, sw, se;   // bilinear weights
    float w, e, n, s;       // fractions
    float mx, my;           // 0 where border padding clamped the position, else 1
    int x0, y0;             // top-left tap (clamped to [-2, size + 1])
    bool in_nw, in_ne, in_sw, in_se;   // in-bounds taps; a non-finite position has none
    __device__ __forceinline__ bool any() const { return in_nw || in_ne || in_sw || in_se; }
};

__device__ __forceinline__ Sample sample(float fx, float fy, int x, int y, const Geometry& g, int pad) {
    Sample q;
    const int H = g.H, W = g.W;
    double ix = ((double)x + (double)fx) * g.rx - 0.5, iy = ((double)y + (double)fy) * g.ry - 0.5;
    const bool finite = fabs(ix) < (double)__builtin_inff() && fabs(iy) < (double)__builtin_inff();   // (false for a NaN)
    if (!finite) ix = iy = 0.0;   // no tap; finite weights, so that 0 texels times them are 0 and not NaN
    q.mx = 1.0f; q.my = 1.0f;
    if (pad == PAD_BORDER) {
        const double cx = fmin(fmax(ix, 0.0), (double)(W - 1)), cy = fmin(fmax(iy, 0.0), (double)(H - 1));
        q.mx = cx == ix ? 1.0f : 0.0f;
        q.my = cy == iy ? 1.0f : 0.0f;
        ix = cx; iy = cy;
    }
    const double xf = floor(ix), yf = floor(iy);
    q.w = (float)(ix - xf); q.e = (float)((xf + 1.0) - ix); q.n = (float)(iy - yf); q.s = (float)((yf + 1.0) - iy);
    q.nw = q.e * q.s; q.ne = q.w * q.s; q.sw = q.e * q.n; q.se = q.w * q.n;
    q.x0 = (int)fmin(fmax(xf, -2.0), (double)(W + 1)); q.y0 = (int)fmin(fmax(yf, -2.0), (double)(H + 1));
    const bool xi0 = q.x0 >= 0 && q.x0 < W, xi1 = q.x0 + 1 >= 0 && q.x0 + 1 < W;
    const bool yi0 = q.y0 >= 0 && q.y0 < H, yi1 = q.y0 + 1 >= 0 && q.y0 + 1 < H;
    q.in_nw = finite && xi0 && yi0; q.in_ne = finite && xi1 && yi0; q.in_sw = finite && xi0 && yi1; q.in_se = finite && xi1 && yi1;
    return q;
}

// a channel's four texels, zeros outside; p: the channel's element (y0, x0), which may lie outside (then not read)
struct Texels {
    float nw, ne, sw, se;
};
__device__ __forceinline__ Texels load(const float* __restrict__ plane, long long tap, const Sample& q, int W) {
    return {q.in_nw ? plane[tap] : 0.0f, q.in_ne ? plane[tap + 1] : 0.0f, q.in_sw ? plane[tap + W] : 0.0f,
            q.in_se ? plane[tap + W + 1] : 0.0f};
}
__device__ __forceinline__ float value(const Sample& q, const Texels& v) {
    return ((v.nw * q.nw + v.ne * q.ne) + v.sw * q.sw) + v.se * q.se;
}
__device__ __forceinline__ float d_ix(const Sample& q, const Texels& v) { return (v.ne - v.nw) * q.s + (v.se - v.sw) * q.n; }
__device__ __forceinline__ float d_iy(const Sample& q, const Texels& v) { return (v.sw - v.nw) * q.e + (v.se - v.ne) * q.w; }

// g w_t to the in-bounds taps of one channel (an in-bounds tap receives g w even when w == 0, an out-of-bounds tap nothing);
// at: the channel's element (y0, x0) of the contiguous [B,C,H,W] gradient, which may lie outside (then unused)
template <class Sink>
__device__ __forceinline__ void scatter(const Sample& q, long long at, int W, float g, Sink& sink) {
    const float qnw = g * q.nw, qne = g * q.ne, qsw = g * q.sw, qse = g * q.se;
    if (q.in_nw) sink.add(at, qnw);
    if (q.in_ne) sink.add(at + 1, qne);
    if (q.in_sw) sink.add(at + W, qsw);
    if (q.in_se) sink.add(at + W + 1, qse);
}

}  // namespace flow
}  // namespace pdepth
