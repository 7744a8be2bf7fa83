// The per-window arithmetic of SSIM (losses/loss_blocks.py:47-66), evaluated by the forward and the backward kernel of ssim.hip:
// both see the same bits of every window, so the backward's clamp decision is the forward's.
//
//   m_x, m_y, e_xx, e_yy, e_xy = window sums / n,  n = (2 md + 1)^2
//   s_x = e_xx - m_x^2,  s_y = e_yy - m_y^2,  s_xy = e_xy - m_x m_y
//   A1 = 2 m_x m_y + C1,  A2 = 2 s_xy + C2,  B1 = m_x^2 + m_y^2 + C1,  B2 = s_x + s_y + C2
//   S = A1 A2 / (B1 B2),  dist = clamp((1 - S) / 2, 0, 1)
//
// A window sum is one running sum over the taps in row-major order, from 0: the order in which ATen's average pooling adds them, so
// the sums -- and with them the whole chain -- have the bits of the reference's float32 composition.  Every operation is a single
// fp32 rounding (the library is built with -ffp-contract=off), the divisions are IEEE divisions.  The form is the reference's symmetric
// one: with x and y equal bit for bit the five sums pair up (e_xx = e_yy = e_xy, m_x = m_y), so A1 == B1, A2 == B2, S == 1 and
// dist == 0 exactly.
//
// Backward.  With G = -1/2 g_out where 0 <= (1 - S) / 2 <= 1 (torch.clamp's inclusive rule) and 0 elsewhere, the gradient of a
// pixel p of the window is (1 / n) G (P + Q x_p + R y_p) for x and (1 / n) G (P' + Q y_p + R x_p) for y, where
//   P = 2 m_y (A2 - A1) / (B1 B2) - S (2 m_x / B1 - 2 m_x / B2),  P' = P with x and y exchanged,  Q = -2 S / B2,  R = 2 A1 / (B1 B2).
// They are evaluated over the common denominator D = B1 B2:
//   P = (2 m_y (A2 - A1) - 2 m_x S (B2 - B1)) / D,  Q = -(2 S B1) / D,  R = (2 A1) / D
// which is the same algebra and keeps the symmetry of the forward: on identical inputs P == 0 and Q == -R bit for bit, so the
// gradient is exactly 0 there instead of the difference of two quotients of the order of 1 / C2.
#pragma once
#include <hip/hip_runtime.h>

namespace pdepth {

namespace {

constexpr float SSIM_C1 = 1e-4f;   // 0.01^2
constexpr float SSIM_C2 = 9e-4f;   // 0.03^2

struct SsimSums {
    float x, y, xx, yy, xy;
};

// the five sums of a K x K window whose rows lie `stride` floats apart: one running sum each, over the taps in row-major order
template <int K>
__device__ __forceinline__ SsimSums ssim_sums(const float* __restrict__ xw, const float* __restrict__ yw, int stride) {
    SsimSums s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < K; ++i) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float a = xw[i * stride + j], b = yw[i * stride + j];
            s.x += a;
            s.y += b;
            s.xx += a * a;
            s.yy += b * b;
            s.xy += a * b;
        }
    }
    return s;
}

struct SsimWindow {
    float mx, my, A1, A2, B1, B2, D, S;
    float d;   // (1 - S) / 2 before the clamp
};

__device__ __forceinline__ SsimWindow ssim_window(const SsimSums& t, float n) {
    SsimWindow w;
    w.mx = t.x / n;
    w.my = t.y / n;
    const float mxy = w.mx * w.my, mxx = w.mx * w.mx, myy = w.my * w.my;
    const float sx = t.xx / n - mxx;
    const float sy = t.yy / n - myy;
    const float sxy = t.xy / n - mxy;
    w.A1 = 2.0f * mxy + SSIM_C1;
    w.A2 = 2.0f * sxy + SSIM_C2;
    w.B1 = (mxx + myy) + SSIM_C1;
    w.B2 = (sx + sy) + SSIM_C2;
    w.D = w.B1 * w.B2;
    w.S = (w.A1 * w.A2) / w.D;
    w.d = (1.0f - w.S) * 0.5f;
    return w;
}

// torch.clamp(0, 1): a NaN stays a NaN
__device__ __forceinline__ float ssim_clamp01(float d) { return d < 0.0f ? 0.0f : (d > 1.0f ? 1.0f : d); }

// G P, G P', G Q, G R of a window
struct SsimCoef {
    float p, pp, q, r;
};

__device__ __forceinline__ SsimCoef ssim_coef(const SsimWindow& w, float g_out) {
    const float G = (w.d >= 0.0f && w.d <= 1.0f) ? -0.5f * g_out : 0.0f;
    const float k = G / w.D;
    const float dA = w.A2 - w.A1;
    const float u = w.S * (w.B2 - w.B1);
    SsimCoef c;
    c.p = k * ((2.0f * w.my) * dA - (2.0f * w.mx) * u);
    c.pp = k * ((2.0f * w.mx) * dA - (2.0f * w.my) * u);
    c.q = -(k * ((2.0f * w.S) * w.B1));
    c.r = k * (2.0f * w.A1);
    return c;
}

}  // namespace

}  // namespace pdepth
