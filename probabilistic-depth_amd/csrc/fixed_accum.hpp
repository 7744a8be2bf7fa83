// Order-independent sums of fp32 contributions: exact integer accumulation.  Users: sweep_bwd_det.hip (exponent from a bound, its
// own policies in sweep_bwd_body.hpp); scatter_det.hip and warp_bwd.hip (exponent from the exact maximum: the sinks,
// max_exponent_pass and max_exponent_scatter below); occlusion.hip (exponent known before the launch: fixed_exponent_scatter);
// inverse_warp.hip and loss_terms.hip take FloatAtomics for the same scatter bodies.
//
// Float addition is not associative, integer addition is.  A contribution q (fp32) is scaled by 2^S (exact: the product is
// formed in double, whose exponent range holds every fp32 times every 2^S chosen below), rounded to the nearest integer, ties to
// even, and added to a 64-bit integer with an integer atomic; a last pass converts the sum back:
//     g = fl32(2^-S * sum_i rn(2^S q_i))
// The result depends on the multiset of the q_i alone -- not on the order of arrival, the scheduling of workgroups or the way
// a kernel stages its adds.
//
// The exponent S is chosen per batch item from a bound M >= |q_i| and the largest number n of contributions one destination
// can receive (det_scale_exponent): n 2 M 2^S <= 2^62, so the sum stays below 2^62 + n / 2 even when every rounding goes
// up and M is a few ulp short, and n M 2^S > 2^58: at most 3 bits of the 62 are wasted.  A destination's absolute error
// is at most n_actual / 2 units of 2^-S, i.e. below 2^-59 n M per contribution actually added.
//
// Conversion (det_to_float): int64 -> double (exact below 2^53, otherwise one rounding to nearest), times 2^-S (exact),
// double -> fp32 (one rounding to nearest): at most two roundings, one fixed instruction sequence.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "kernels.hpp"   // launch_zero (clear.hip)

namespace pdepth {
namespace fixed {

// the two answers of det_scale_exponent that are no exponent (every exponent lies in [-200, 300])
constexpr int32_t EXP_ZERO = INT32_MIN;        // bound == 0: every contribution is 0
constexpr int32_t EXP_NONFINITE = INT32_MAX;   // bound is NaN or infinite

__host__ __device__ inline uint32_t float_bits(float x) {
    union { float f; uint32_t u; } v;
    v.f = x;
    return v.u;
}

// S with n 2 bound 2^S <= 2^62 < 16 n bound 2^S, for a finite bound > 0 (denormals included) and n >= 1; integer arithmetic on
// the bit pattern of the bound only: the host and the device give the same answer.
//   bound < 2^em, bound >= 2^(em - 1);  n <= 2^en, n > 2^(en - 1)  =>  S = 61 - em - en: n 2 bound 2^S <= 2^62, n bound 2^S > 2^59
__host__ __device__ inline int32_t det_scale_exponent(float bound, int64_t n) {
    const uint32_t bits = float_bits(bound) & 0x7fffffffu;
    if (bits == 0u) return EXP_ZERO;
    if (bits >= 0x7f800000u) return EXP_NONFINITE;
    const int field = (int)(bits >> 23);
    const int em = field != 0 ? field - 126 : (32 - __builtin_clz(bits)) - 149;   // (field 0: bits is the mantissa, bound = bits 2^-149)
    const int en = n > 1 ? 64 - __builtin_clzll((unsigned long long)(n - 1)) : 0;
    return 61 - em - en;
}

// |x| as an unsigned integer: ordered like |x| for finite values, every infinity above them and every NaN above the infinities --
// a maximum over these (atomicMax) is order-independent and a NaN or infinity anywhere wins it
__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ bool bits_finite(uint32_t abs_bits_of_x) { return abs_bits_of_x < 0x7f800000u; }

// maximum of v over the 64 lanes of a wave (every lane calls; dead lanes pass 0)
__device__ __forceinline__ uint32_t wave_max_bits(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// the maximum of a wave's |q| bits into an item's header word (every lane of the wave calls)
__device__ __forceinline__ void put_max(uint32_t m, uint32_t* __restrict__ slot) {
    m = wave_max_bits(m);
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(slot, m);
}

// the exponent of a scatter whose header word of an item is the exact maximum of |q| over its contributions (max_exponent_pass);
// n: the most contributions one destination can receive
struct MaxExponent {
    static constexpr int WORDS = 1;
    long long n;
    __device__ int operator()(const uint32_t* h) const { return det_scale_exponent(__uint_as_float(h[0]), n); }
};

// rn(2^S q): the product is exact in double, the rounding is to nearest, ties to even
__device__ __forceinline__ long long det_quantise(float q, int S) { return (long long)__builtin_rint(__builtin_ldexp((double)q, S)); }

// quantise and add: one ds_add_u64 on LDS, one global_atomic_add_x2 on global memory (two's complement: unsigned adds)
__device__ __forceinline__ void det_add(unsigned long long* dst, float q, int S) { atomicAdd(dst, (unsigned long long)det_quantise(q, S)); }

// the sum back in fp32 (two roundings at most, see above)
__device__ __forceinline__ float det_to_float(long long acc, int S) { return (float)__builtin_ldexp((double)acc, -S); }

// ---- the sinks of a scatter body: where a contribution q to element `at` of the gradient goes.  A body written against
// add(long long at, float q) forms the same q, bit for bit, on the atomic path and in both passes of the integer sum. ------------
struct FloatAtomics {   // atomicAdd(float*) into the gradient, zeroed first: the last bits depend on the order of arrival
    float* __restrict__ dst;
    __device__ __forceinline__ void add(long long at, float q) { atomicAdd(dst + at, q); }
};
struct MaxOfAbs {   // pass 0: the maximum of |q| of this lane
    uint32_t m;
    __device__ __forceinline__ void add(long long, float q) { m = max(m, abs_bits(q)); }
};
struct IntegerSum {   // pass 1: rn(2^S q) into the int64 accumulator
    unsigned long long* __restrict__ acc;
    int S;   // the exponent of the workgroup's batch item
    __device__ __forceinline__ void add(long long at, float q) { det_add(acc + at, q, S); }
};

// One pass of a max-exponent scatter for this workgroup's batch item: body(sink) hands the lane's contributions to sink.add.
//   PASS 0  the maximum of |q| into the item's header word (atomicMax: order-independent, a NaN or an infinity wins it);
//   PASS 1  S = det_scale_exponent(header, n), n the most contributions one destination can receive, then the same contributions
//           quantised with S and added to acc.
// Every lane of every wave of the workgroup must reach this call: put_max shuffles across the wave, so a lane without a pixel
// runs the body on a shadow pixel and adds nothing instead of returning early.  On a non-exponent (EXP_ZERO, EXP_NONFINITE) the
// whole workgroup leaves -- the exponent is per item and a workgroup serves one item -- and the convert pass writes that item.
template <int PASS, class Body>
__device__ __forceinline__ void max_exponent_pass(uint32_t* __restrict__ item_header, unsigned long long* __restrict__ acc, long long n,
                                                  Body body) {
    if (PASS == 0) {
        MaxOfAbs sink{0u};
        body(sink);
        put_max(sink.m, item_header);
    } else {
        const int S = det_scale_exponent(__uint_as_float(*item_header), n);
        if (S == EXP_ZERO || S == EXP_NONFINITE) return;
        IntegerSum sink{acc, S};
        body(sink);
    }
}

// ---- the workspace of an integer sum: a 256-byte-rounded header of `words` uint32 per batch item (the maxima the exponent is
// derived from), then one int64 per element of the result, [B][per_item] --------------------------------------------------------
inline size_t det_header_bytes(int B, int words) { return ((size_t)B * words * sizeof(uint32_t) + 255) / 256 * 256; }
inline size_t det_workspace_bytes(int B, int words, size_t per_item) {
    return det_header_bytes(B, words) + ((size_t)B * per_item * sizeof(long long) + 255) / 256 * 256;
}
inline unsigned long long* det_accumulator(void* workspace, int B, int words) {
    return reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + det_header_bytes(B, words));
}

// accumulator -> fp32.  Exponent: WORDS (header words per item) and int operator()(const uint32_t* item_header), the S the scatter
// used for the item; an item of EXP_ZERO is 0, an item of EXP_NONFINITE is NaN in every element.
// grid (blocks of 256 elements of an item, B)
template <class Exponent>
__global__ __launch_bounds__(256) void det_convert_kernel(Exponent exponent, const uint32_t* __restrict__ hdr, const long long* __restrict__ acc,
                                                          float* __restrict__ out, size_t per_item) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_item) return;
    const int b = blockIdx.y;
    const int S = exponent(hdr + Exponent::WORDS * b);
    const size_t at = (size_t)b * per_item + i;
    out[at] = S == EXP_ZERO ? 0.0f : S == EXP_NONFINITE ? __uint_as_float(0x7fc00000u) : det_to_float(acc[at], S);
}

// (returns the error of a launch before it, if one is pending, without launching)
template <class Exponent>
inline hipError_t det_convert(void* workspace, int B, size_t per_item, Exponent exponent, float* out, hipStream_t stream) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(det_convert_kernel<Exponent>, dim3((unsigned)((per_item + 255) / 256), B), dim3(256), 0, stream, exponent,
                       static_cast<const uint32_t*>(workspace),
                       reinterpret_cast<const long long*>(det_accumulator(workspace, B, Exponent::WORDS)), out, per_item);
    return hipGetLastError();
}

// The host side of a max-exponent scatter: clear the workspace (header and accumulator), pass 0, pass 1, convert into `out`
// [B][per_item].  launch(pass, hdr, acc) launches the gradient's kernel of pass decltype(pass)::value, whose workgroups call
// max_exponent_pass<PASS>(hdr + b, acc, n, ...) with the same n: kernel and caller take it from one function of the gradient's,
// since a scatter and a convert that disagree on it differ by a power of two, silently.  The caller has checked the workspace
// (det_workspace_bytes(B, MaxExponent::WORDS, per_item)); nothing else clears it.
template <class Launch>
inline hipError_t max_exponent_scatter(void* workspace, int B, size_t per_item, long long n, float* out, hipStream_t stream,
                                       Launch launch) {
    hipError_t e = launch_zero(workspace, det_workspace_bytes(B, MaxExponent::WORDS, per_item), stream);
    if (e != hipSuccess) return e;
    uint32_t* hdr = static_cast<uint32_t*>(workspace);
    unsigned long long* acc = det_accumulator(workspace, B, MaxExponent::WORDS);
    launch(std::integral_constant<int, 0>{}, hdr, acc);
    launch(std::integral_constant<int, 1>{}, hdr, acc);
    return det_convert(workspace, B, per_item, MaxExponent{n}, out, stream);
}

// ---- a scatter whose exponent is known before the launch (occlusion.hip: every contribution lies in [0, 1]) --------------------
// No header, no pass 0: the workspace is the accumulator alone (WORDS == 0), and S = det_scale_exponent(bound, n) is computed by the
// caller on the host, once, for every item.
struct FixedExponent {
    static constexpr int WORDS = 0;
    int S;
    __host__ __device__ int operator()(const uint32_t*) const { return S; }
};

// The host side of a fixed-exponent scatter: clear the accumulator, one pass.  launch(sink) launches the kernel, whose lanes hand
// their contributions to sink.add; the convert pass is the caller's (det_convert with FixedExponent{S}, or a kernel of its own
// that reads det_accumulator(workspace, B, FixedExponent::WORDS) with det_to_float(., S)).  The caller has checked the workspace
// (det_workspace_bytes(B, FixedExponent::WORDS, per_item)) and that S is an exponent.
template <class Launch>
inline hipError_t fixed_exponent_scatter(void* workspace, int B, size_t per_item, int S, hipStream_t stream, Launch launch) {
    hipError_t e = launch_zero(workspace, det_workspace_bytes(B, FixedExponent::WORDS, per_item), stream);
    if (e != hipSuccess) return e;
    launch(IntegerSum{det_accumulator(workspace, B, FixedExponent::WORDS), S});
    return hipGetLastError();
}

}  // namespace fixed
}  // namespace pdepth
