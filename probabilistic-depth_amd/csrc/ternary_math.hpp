// The chain of one (centre, neighbour) pair of the ternary census distance (losses/loss_blocks.py:8-44), stated once for the
// forward and the backward of ternary.hip.  With t = I(neighbour) - I(centre) of the first image and t' of the second:
//     n = t / sqrt(0.81 + t^2)      d = (n - n')^2      h = d / (0.1 + d)
// in the reference's order of operations: correctly rounded sqrt and division, no contraction (-ffp-contract=off), so n, d and h
// have the reference's float32 bits.  Where the two images are equal bit for bit, n == n', d = 0, h = 0 and both derivatives are 0.
//
// The derivatives, from dn/dt = 0.81 / s^3 (s = sqrt(0.81 + t^2)) and dh/dd = 0.1 / (0.1 + d)^2:
//     dh/dt  =  a * 0.81 / s^3        dh/dt' = -a * 0.81 / s'^3        a = 0.2 (n - n') / (0.1 + d)^2
// The closed form 0.81 / s^3 has no cancellation; autograd's 1 / s - t (t / s^2) / s loses up to |t|^2 / 0.81 of its precision.
//
// h is even in (t, t') jointly and its derivatives are odd: the pair (p, q) seen from q has t and t' negated, the same h and the
// negated derivatives, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace pdepth {

// (r * 0.2989 + g * 0.5870 + b * 0.1140) * 255, left to right
__device__ __forceinline__ float ternary_gray255(float r, float g, float b) {
    return ((r * 0.2989f + g * 0.5870f) + b * 0.1140f) * 255.0f;
}

__device__ __forceinline__ float ternary_h(float t, float tp) {
    const float n = t / sqrtf(0.81f + t * t);
    const float np = tp / sqrtf(0.81f + tp * tp);
    const float e = n - np;
    const float d = e * e;
    return d / (0.1f + d);
}

struct TernaryDeriv {
    float dt, dtp;   // dh/dt, dh/dt'
};

__device__ __forceinline__ TernaryDeriv ternary_deriv(float t, float tp) {
    const float u = 0.81f + t * t, up = 0.81f + tp * tp;
    const float s = sqrtf(u), sp = sqrtf(up);
    const float e = t / s - tp / sp;
    const float q = 0.1f + e * e;
    const float a = (0.2f * e) / (q * q);
    return {a * (0.81f / (u * s)), -(a * (0.81f / (up * sp)))};
}

}  // namespace pdepth
