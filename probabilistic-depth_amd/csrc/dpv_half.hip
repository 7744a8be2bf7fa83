// The DPV reductions on fp16 / bf16 logits: pdepth_dpv_reduce_ex_lp, pdepth_dpv_reduce_backward_lp (include/pdepth.h).
//
// Under torch.autocast the conv stacks hand over half-precision logits.  A cast in front of the fp32 reduction is one more pass
// over the largest tensor of a step; here the cast is the load (forward: 6 bytes per element with logp, against 14) or the
// store (backward: 10 against 18).  The bodies are those of dpv.hip and dpv_bwd.hip (dpv_reduce_body.hpp): a value is widened
// to fp32 where it is loaded, which is exact, and every operation after that is the fp32 kernel's in its order, so the fp32
// outputs have the bits of the fp32 entry on the widened input.  prob (on request) and g_logits are rounded to nearest-even
// from the fp32 value where they are stored.  The log-DPV stays fp32: nothing downstream has a second element type.
//
// Forward, wave layout (dpv_lanes.hpp): a lane's quad of 4 pixels is one 8-byte non-temporal load.  What the layout does not
// take -- D > 128, W % 4 != 0, or a base address that is not 8-byte aligned (a 2-byte view may start 2 bytes into its storage)
// -- runs one pixel per thread.  There the sums run in ascending planes, as in the fp32 any-shape kernel, except when only an
// address keeps the volume out of the wave layout: then in the wave layout's order (plane_sum), since the fp32 entry on the
// widened copy, which is aligned, would run the wave layout.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "dpv_lanes.hpp"
#include "dpv_reduce_body.hpp"

namespace pdepth {

namespace {

template <typename X, typename P, int RPL>
__global__ __launch_bounds__(256) void dpv_reduce_lp_vec4_kernel(const X* __restrict__ x, const float* __restrict__ dc, int D, int HW,
                                                                 float* logp, float* __restrict__ depth, DpvExtrasAs<X, P> ex) {
    dpv_reduce_lanes<RPL, true>(x, dc, D, HW, logp, depth, ex);
}

template <typename X, typename P, bool LANES>
__global__ __launch_bounds__(256) void dpv_reduce_lp_pixel_kernel(const X* x, const float* __restrict__ dc, int D, int HW, float* logp,
                                                                  float* __restrict__ depth, DpvExtrasAs<X, P> ex) {
    dpv_reduce_ex_pixel<LANES>(x, dc, D, HW, logp, depth, ex);
}

template <typename GX, typename GP>
__global__ __launch_bounds__(256) void dpv_reduce_lp_bwd_kernel(const float* __restrict__ logp, const float* __restrict__ dc, int D, int HW,
                                                                const float* __restrict__ g_logp, const GP* __restrict__ g_prob,
                                                                const float* __restrict__ g_depth, GX* __restrict__ g_x) {
    dpv_reduce_bwd_pixel(logp, dc, D, HW, g_logp, g_prob, g_depth, g_x);
}

template <typename X, typename P>
hipError_t launch_reduce_lp(const void* logits, const void* addend, const float* d_candi, int B, int D, int H, int W, float* logp,
                            void* prob, float* depth, float* variance, float* quarter, hipStream_t stream) {
    const int HW = H * W;
    const X* x = static_cast<const X*>(logits);
    DpvExtrasAs<X, P> ex{static_cast<const X*>(addend), static_cast<P*>(prob), variance, quarter, W};
    const bool shape = (W % 4 == 0) && D <= 128;
    const bool at_quads = aligned8(logits) && (!addend || aligned8(addend)) && (!logp || aligned16(logp)) &&
                          (!prob || (sizeof(P) == 4 ? aligned16(prob) : aligned8(prob))) && (!depth || aligned16(depth)) &&
                          (!variance || aligned16(variance));
    const dim3 grid(n_blocks(H, W), B);
    if (shape && at_quads) {
        for_planes_per_lane(D, [&](auto rpl) {
            hipLaunchKernelGGL((dpv_reduce_lp_vec4_kernel<X, P, decltype(rpl)::value>), grid, dim3(256), 0, stream, x, d_candi, D, HW, logp,
                               depth, ex);
        });
    } else if (shape) {
        hipLaunchKernelGGL((dpv_reduce_lp_pixel_kernel<X, P, true>), grid, dim3(256), 0, stream, x, d_candi, D, HW, logp, depth, ex);
    } else {
        hipLaunchKernelGGL((dpv_reduce_lp_pixel_kernel<X, P, false>), grid, dim3(256), 0, stream, x, d_candi, D, HW, logp, depth, ex);
    }
    return hipGetLastError();
}

template <typename GX, typename GP>
hipError_t launch_bwd_lp(const float* logp, const float* d_candi, int B, int D, int H, int W, const float* g_logp, const void* g_prob,
                         const float* g_depth, void* g_logits, hipStream_t stream) {
    const int HW = H * W;
    hipLaunchKernelGGL((dpv_reduce_lp_bwd_kernel<GX, GP>), dim3((HW + 255) / 256, B), dim3(256), 0, stream, logp, d_candi, D, HW, g_logp,
                       static_cast<const GP*>(g_prob), g_depth, static_cast<GX*>(g_logits));
    return hipGetLastError();
}

}  // namespace

}  // namespace pdepth

using namespace pdepth::capi;

extern "C" {

int pdepth_dpv_reduce_ex_lp(int32_t dtype, const void* logits, const void* addend, const float* d_candi, int32_t B, int32_t D,
                            int32_t H, int32_t W, float* logp, void* prob, int32_t prob_is_lp, float* depth, float* variance,
                            float* logp_quarter, void* stream) {
    const char* who = "pdepth_dpv_reduce_ex_lp";
    if (dtype != PDEPTH_DTYPE_F16 && dtype != PDEPTH_DTYPE_BF16)
        return fail(PDEPTH_E_ARG, "%s: unknown dtype %d (PDEPTH_DTYPE_F16 or PDEPTH_DTYPE_BF16)", who, dtype);
    if (!logits || !d_candi) return fail(PDEPTH_E_ARG, "%s: null input", who);
    if (!logp && !prob && !depth && !variance && !logp_quarter) return fail(PDEPTH_E_ARG, "%s: no output requested", who);
    if (int rc = check_dims(who, B, D, H, W)) return rc;
    if (int rc = check_launch_limits(who, B, H, W)) return rc;
    if (logp_quarter && (H < 4 || W < 4)) return fail(PDEPTH_E_ARG, "%s: quarter output needs H, W >= 4", who);
    if ((const void*)logp == logits || prob == logits || (const void*)variance == logits ||
        (addend && ((const void*)logp == addend || prob == addend)))
        return fail(PDEPTH_E_ARG, "%s: no output may alias the half-precision logits or addend", who);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    using pdepth::bf16_t;
    using pdepth::f16_t;
    if (dtype == PDEPTH_DTYPE_F16)
        e = prob_is_lp ? pdepth::launch_reduce_lp<f16_t, f16_t>(logits, addend, d_candi, B, D, H, W, logp, prob, depth, variance, logp_quarter, s)
                       : pdepth::launch_reduce_lp<f16_t, float>(logits, addend, d_candi, B, D, H, W, logp, prob, depth, variance, logp_quarter, s);
    else
        e = prob_is_lp ? pdepth::launch_reduce_lp<bf16_t, bf16_t>(logits, addend, d_candi, B, D, H, W, logp, prob, depth, variance, logp_quarter, s)
                       : pdepth::launch_reduce_lp<bf16_t, float>(logits, addend, d_candi, B, D, H, W, logp, prob, depth, variance, logp_quarter, s);
    return launched(e, who);
}

int pdepth_dpv_reduce_backward_lp(int32_t dtype, const float* logp, const float* d_candi, int32_t B, int32_t D, int32_t H, int32_t W,
                                  const float* g_logp, const void* g_prob, int32_t g_prob_is_lp, const float* g_depth, void* g_logits,
                                  void* stream) {
    const char* who = "pdepth_dpv_reduce_backward_lp";
    if (dtype != PDEPTH_DTYPE_F16 && dtype != PDEPTH_DTYPE_BF16)
        return fail(PDEPTH_E_ARG, "%s: unknown dtype %d (PDEPTH_DTYPE_F16 or PDEPTH_DTYPE_BF16)", who, dtype);
    if (!logp || !d_candi || !g_logits) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!g_logp && !g_prob && !g_depth) return fail(PDEPTH_E_ARG, "%s: no incoming gradient", who);
    if (int rc = check_dims(who, B, D, H, W)) return rc;
    if (int rc = check_launch_limits(who, B, H, W)) return rc;
    if ((const void*)g_logits == logp || (const void*)g_logits == g_logp || (g_prob && (const void*)g_logits == g_prob))
        return fail(PDEPTH_E_ARG, "%s: g_logits may alias no input", who);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    using pdepth::bf16_t;
    using pdepth::f16_t;
    if (dtype == PDEPTH_DTYPE_F16)
        e = g_prob_is_lp ? pdepth::launch_bwd_lp<f16_t, f16_t>(logp, d_candi, B, D, H, W, g_logp, g_prob, g_depth, g_logits, s)
                         : pdepth::launch_bwd_lp<f16_t, float>(logp, d_candi, B, D, H, W, g_logp, g_prob, g_depth, g_logits, s);
    else
        e = g_prob_is_lp ? pdepth::launch_bwd_lp<bf16_t, bf16_t>(logp, d_candi, B, D, H, W, g_logp, g_prob, g_depth, g_logits, s)
                         : pdepth::launch_bwd_lp<bf16_t, float>(logp, d_candi, B, D, H, W, g_logp, g_prob, g_depth, g_logits, s);
    return launched(e, who);
}

}  // extern "C"
