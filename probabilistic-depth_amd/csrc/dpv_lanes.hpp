// The wave layout of the kernels that read a [B,D,H,W] volume once and reduce it over D: dpv.hip (log-softmax + expectation),
// dpv_half.hip (the same on fp16 / bf16 logits: a quad is then one 8-byte access), loss.hip (soft-label cross-entropy) and
// metrics.hip (volume form).  This is the one description of it.
//
// A workgroup is 4 waves and covers 256 consecutive pixels of one item (blockIdx.y); a wave covers 64 of them.
//   lane = (plane group g = lane >> 4, pixel quad q = lane & 15).  A quad is 4 consecutive pixels, one 16-byte access; the 16
//   quads of a wave cover 256 contiguous bytes of every plane row.
//   The 4 plane groups interleave the D planes: group g holds planes k = g + 4 i, i < N (N planes per lane: 8, 16 or 32 for
//   D <= 32, 64, 128 -- for_planes_per_lane).  A plane with k >= D, and every plane of a lane past the last quad (not live),
//   is a fill value the caller chooses; such a lane reads nothing and writes nothing.
//   The volume is read once and written once: non-temporal 16-byte accesses (+5 % measured), a lane's loads issued together.
//   Per-pixel partial results of the 4 plane groups are combined over lanes l, l^16, l^32, l^48 (group_sum, group_max): two
//   xor-shuffles, after which every plane group holds the result of all four pixels of its quad.
// Seen per pixel, lane (g, q) of wave w stands for pixel 64 w + 4 q + g of the workgroup's 256 (thread_pixel): the kernels
// that evaluate one pixel per thread beside a wave-layout kernel use this mapping, so that both feed a workgroup sum alike.
//
// Bit-equal results come from here, not from look-alike loops: the expectation sum_k d_k (exp) v_k of the loss, the metrics and
// the reductions has one definition (expect_add, expect_planes -- products d_k * value, planes in ascending i, plane groups by
// group_sum), and so has the sum over the threads of a workgroup (wg_sum_put / wg_sum_get: lanes by xor 32 ... 1, then
// (w0 + w1) + (w2 + w3) through LDS).  Two pieces are written out where they are used because the helpers cost them time
// (profiles/r11_dpv_lanes/README.md): the load loop of dpv_expect_vec4_kernel (dpv.hip) and the ten-sum record of metrics.hip.
// Every object is built with -ffp-contract=off: the same operations in the same order give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace pdepth {

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 load_nt(const float* p) {
    const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ void store_nt(float* p, float4 v) {
    __builtin_nontemporal_store(v4f{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f*>(p));
}
// The 2-byte element types a reduction may read its logits in or write prob / a gradient in (dpv_half.hip); everything between
// the load and the store is fp32.  Widening is exact; narrowing rounds to nearest-even (overflow to inf, NaN stays NaN): the
// compiler's conversions, v_cvt_f16_f32 and on gfx950 v_cvt_pk_bf16_f32 (the integer form of the bf16 rounding cost the 8-plane
// kernel two registers, and with them a wave per SIMD).
struct f16_t { uint16_t bits; };    // IEEE binary16
struct bf16_t { uint16_t bits; };   // bfloat16: the upper half of a binary32
__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(f16_t h) { return (float)__builtin_bit_cast(_Float16, h.bits); }
__device__ __forceinline__ float widen(bf16_t h) { return __uint_as_float((uint32_t)h.bits << 16); }
template <typename T>
__device__ __forceinline__ T narrow(float v);
template <>
__device__ __forceinline__ float narrow<float>(float v) { return v; }
template <>
__device__ __forceinline__ f16_t narrow<f16_t>(float v) { return f16_t{__builtin_bit_cast(uint16_t, (_Float16)v)}; }
template <>
__device__ __forceinline__ bf16_t narrow<bf16_t>(float v) {
    return bf16_t{__builtin_bit_cast(uint16_t, (__bf16)v)};
}
// a quad of 2-byte elements: one 8-byte non-temporal access (the pointer 8-byte aligned)
typedef uint32_t v2u __attribute__((ext_vector_type(2)));
template <typename T, typename = std::enable_if_t<sizeof(T) == 2>>
__device__ __forceinline__ float4 load_nt(const T* p) {
    const v2u t = __builtin_nontemporal_load(reinterpret_cast<const v2u*>(p));
    return make_float4(widen(T{(uint16_t)(t.x & 0xffffu)}), widen(T{(uint16_t)(t.x >> 16)}), widen(T{(uint16_t)(t.y & 0xffffu)}),
                       widen(T{(uint16_t)(t.y >> 16)}));
}
template <typename T, typename = std::enable_if_t<sizeof(T) == 2>>
__device__ __forceinline__ void store_nt(T* p, float4 v) {
    const v2u t = {(uint32_t)narrow<T>(v.x).bits | ((uint32_t)narrow<T>(v.y).bits << 16),
                   (uint32_t)narrow<T>(v.z).bits | ((uint32_t)narrow<T>(v.w).bits << 16)};
    __builtin_nontemporal_store(t, reinterpret_cast<v2u*>(p));
}
__device__ __forceinline__ float4 shfl_xor4(float4 v, int m) {
    return make_float4(__shfl_xor(v.x, m), __shfl_xor(v.y, m), __shfl_xor(v.z, m), __shfl_xor(v.w, m));
}
__device__ __forceinline__ float4 splat4(float s) { return make_float4(s, s, s, s); }

// over the 4 plane groups of a wave
__device__ __forceinline__ float4 group_sum(float4 v) {
#pragma unroll
    for (int s = 16; s <= 32; s <<= 1) {
        const float4 o = shfl_xor4(v, s);
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    return v;
}
__device__ __forceinline__ float4 group_max(float4 v) {
#pragma unroll
    for (int s = 16; s <= 32; s <<= 1) {
        const float4 o = shfl_xor4(v, s);
        v.x = fmaxf(v.x, o.x); v.y = fmaxf(v.y, o.y); v.z = fmaxf(v.z, o.z); v.w = fmaxf(v.w, o.w);
    }
    return v;
}

struct QuadLane {
    int g, q, b;   // plane group, pixel quad within the item, item
    bool live;     // the quad exists (q < HW / 4)
    size_t off;    // of the quad in plane 0 of item b of a [B,D,H,W] volume (quad 0 for a lane that is not live)
    size_t poff;   // of the quad in item b of a [B,H,W] map (past the item for a lane that is not live: load_quad)
};
__device__ __forceinline__ QuadLane quad_lane(int D, int HW) {
    QuadLane L;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    L.g = lane >> 4;
    L.q = wave * 16 + (lane & 15);
    L.live = L.q < (HW >> 2);
    L.b = blockIdx.y;
    L.off = (size_t)L.b * D * HW + (size_t)(L.live ? L.q : 0) * 4;
    L.poff = (size_t)L.b * HW + (size_t)L.q * 4;
    return L;
}
// the same layout per pixel: the pixel of this thread within its item
__device__ __forceinline__ int thread_pixel() {
    const int lane = threadIdx.x & 63;
    return blockIdx.x * 256 + (threadIdx.x >> 6) * 64 + (lane & 15) * 4 + (lane >> 4);
}

// the lane's quad of a [B,H,W] map
__device__ __forceinline__ float4 load_quad(const float* map, const QuadLane& L, float fill) {
    return L.live ? *reinterpret_cast<const float4*>(map + L.poff) : splat4(fill);
}

// planes g + 4 (c0 + u), u < N, of the lane's quad [+ the same planes of `add`]; `fill` where there is no such plane to read
// (T: float, or a 2-byte element type widened at the load)
template <int N, typename T>
__device__ __forceinline__ void load_planes(float4 (&v)[N], const T* x, const QuadLane& L, int c0, int D, int HW, float fill,
                                            bool wanted = true, const T* add = nullptr) {
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const int k = L.g + 4 * (c0 + u);
        const bool ok = k < D && L.live && wanted;
        v[u] = ok ? load_nt(x + L.off + (size_t)k * HW) : splat4(fill);
        if (add && ok) {
            const float4 a = load_nt(add + L.off + (size_t)k * HW);
            v[u].x += a.x; v[u].y += a.y; v[u].z += a.z; v[u].w += a.w;
        }
    }
}

// the expectation: e += d_k * (exp) v for one plane of a quad, and for the N planes of a lane from chunk c0 on
template <bool BV_LOG>
__device__ __forceinline__ void expect_add(float4& e, float dk, const float4& v) {
    e.x += dk * (BV_LOG ? expf(v.x) : v.x); e.y += dk * (BV_LOG ? expf(v.y) : v.y);
    e.z += dk * (BV_LOG ? expf(v.z) : v.z); e.w += dk * (BV_LOG ? expf(v.w) : v.w);
}
template <bool BV_LOG, int N>
__device__ __forceinline__ void expect_planes(float4& e, const float4 (&v)[N], const float* dc, int g, int c0, int D) {
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const int k = g + 4 * (c0 + u);
        if (k < D) expect_add<BV_LOG>(e, dc[k], v[u]);
    }
}

// The sum over the 256 threads of a workgroup in a fixed order, in two halves around the caller's one __syncthreads():
// put = the lanes of a wave by xor-shuffles 32 ... 1, lane 0 of wave w writes s[w]; get = (s[0] + s[1]) + (s[2] + s[3]).
template <typename T>
__device__ __forceinline__ void wg_sum_put(T v, T (&s)[4]) {
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) v = v + __shfl_xor(v, sh);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
}
template <typename T>
__device__ __forceinline__ T wg_sum_get(const T (&s)[4]) {
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// workgroups of 256 pixels per item
inline int n_blocks(int H, int W) { return (int)(((long long)H * W + 255) / 256); }

// planes per lane from D (D <= 128): f(std::integral_constant<int, 8 | 16 | 32>)
template <typename F>
inline void for_planes_per_lane(int D, F&& f) {
    if (D <= 32) f(std::integral_constant<int, 8>{});
    else if (D <= 64) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 32>{});
}

}  // namespace pdepth
