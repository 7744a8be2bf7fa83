// g_src of the plane-sweep backward as an order-independent sum: the same bits from call to call, whatever the order in which
// the adds arrive, however the planes are grouped, whichever other items share the batch.
//
// The contributions are those of the g_src pass of sweep_bwd.hip, bit for bit, by construction: both kernels are the one body of
// sweep_bwd_body.hpp (sample positions and footprints, the per-channel chain, the 16 x 16 tiles, per-plane boxes, plane groups
// staged through an LDS box image, direct adds for a plane whose box alone exceeds the cap, the channel tail).  What differs is
// the policy (sweep_bwd::IntegerSum, over fixed_accum.hpp): a contribution q is scaled by 2^S_b, rounded to an integer and added
// with integer atomics -- ds_add_u64 into the box image, global_atomic_add_x2 into the accumulator of the workspace --, 4 channels per pass,
// and a last pass converts the accumulator into g_src.
//
// Launch sequence, all on the caller's stream, no host synchronisation, no copy to the host:
//   1. zero fill (clear.hip) of the workspace (the per-item header and the accumulator);
//   2. bounds pre-pass: per item max |g_cost[b]| and, for L2, max |src[b]| and max |ref[b]|, as atomicMax over the bit patterns
//      of |x| (order-independent; a NaN or an infinity wins the maximum);
//   3. scatter (L2 / L1).  Every workgroup derives S_b of its item from the header (ItemExponent: a few integer operations):
//      M_b = |gscale| max|g_cost[b]| E_b bounds every contribution, E_b = max|src[b]| + max|ref[b]| for L2 and 1 for L1, and a
//      texel receives at most N = D H W contributions (per view, a (plane, pixel) sample puts at most one tap, of weight <= 1,
//      on it);
//   4. convert: accumulator -> fp32.  An item whose M_b is 0 is 0.  An item whose bound is not finite -- a NaN or an infinity
//      in g_cost[b] (or, L2, in src[b] / ref[b]), or a factor of M_b (or M_b itself) at or above 2^127, where the fp32 chain is
//      no longer certain to stay finite -- is NaN in every element: an integer cannot hold a NaN, and a non-finite gradient
//      anywhere in an item is what an overflow check of the caller looks for.  (The atomic path confines a NaN to the texels it
//      reaches.)  Every other item is untouched by it.
//
// Workspace: 256-byte-rounded header of 16 bytes per item, then one int64 per element of g_src: 8 B V C H W bytes (B = 4, V = 1,
// C = 67: 17.6 MB at 64 x 128, 281 MB at 256 x 512).
//
// LDS: the box image holds 64-bit integers: BCC * BOX_CAP * 8 bytes = 64 KB at BCC = 4, + 64 D bytes of boxes (96 KB at D = 512).
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "fixed_accum.hpp"
#include "kernels.hpp"
#include "sweep_bwd_body.hpp"

namespace pdepth {

namespace {

using namespace fixed;
using namespace sweep_bwd;

// S_b (or EXP_ZERO / EXP_NONFINITE) from the maxima of an item; the scatter and the convert kernel evaluate it on the same words
struct ItemExponent {
    static constexpr int WORDS = 4;   // per item: bits of max |g_cost|, max |src|, max |ref|, unused
    float gscale;
    int metric;
    long long n;   // the most contributions a texel can receive
    __host__ __device__ ItemExponent(const SweepArgs& a, int metric_)
        : gscale((metric_ == 0 ? 2.0f : 1.0f) / a.sigma), metric(metric_), n((long long)a.D * (a.H * a.W)) {}
    __device__ int operator()(const uint32_t* __restrict__ h) const {
        const uint32_t gb = h[0], sb = h[1], rb = h[2];
        if (!bits_finite(gb) || (metric == 0 && (!bits_finite(sb) || !bits_finite(rb)))) return EXP_NONFINITE;
        const double limit = 0x1p127;
        const double coef = (double)fabsf(gscale) * (double)__uint_as_float(gb);
        const double e = metric == 0 ? (double)__uint_as_float(sb) + (double)__uint_as_float(rb) : 1.0;
        const double m = coef * e;   // (three fp32 factors: no underflow, no overflow in double)
        if (!(coef < limit && e < limit && m < limit)) return EXP_NONFINITE;
        if (m == 0.0) return EXP_ZERO;
        const float bound = (float)m;
        return det_scale_exponent(bound > 0.0f ? bound : __uint_as_float(1u), n);   // (below the smallest denormal: that one)
    }
};
constexpr int HDR_WORDS = ItemExponent::WORDS;

// grid (blocks, B, 1 | 3): z = 0 g_cost[b] (D H W), 1 src[b] (V views of C H W), 2 ref[b] (C H W)
__global__ __launch_bounds__(256) void sweep_det_bounds_kernel(SweepArgs a, const float* __restrict__ gcost, uint32_t* __restrict__ hdr) {
    const int b = blockIdx.y, which = blockIdx.z;
    const size_t HW = (size_t)a.H * a.W;
    const size_t chw = (size_t)a.C * HW;
    const float* base = which == 0 ? gcost + (size_t)b * a.D * HW : which == 1 ? a.src + (size_t)b * a.src_bstride : a.ref + (size_t)b * a.ref_bstride;
    const size_t n = which == 0 ? (size_t)a.D * HW : chw;
    const int views = which == 1 ? a.V : 1;
    uint32_t m = 0u;
    for (int v = 0; v < views; ++v) {
        const float* p = base + (size_t)v * a.src_vstride;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = max(m, abs_bits(p[i]));
    }
    m = wave_max_bits(m);
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(hdr + HDR_WORDS * b + which, m);
}

template <int METRIC>
__global__ __launch_bounds__(BTHREADS) void sweep_bwd_det_kernel(SweepArgs a, const float* __restrict__ gcost, const uint32_t* __restrict__ hdr,
                                                                 unsigned long long* __restrict__ acc) {
    const int S = ItemExponent(a, METRIC)(hdr + HDR_WORDS * blockIdx.y);
    if (S == EXP_ZERO || S == EXP_NONFINITE) return;   // (the whole workgroup: the convert pass writes this item)
    sweep_bwd_body<METRIC, false>(a, gcost, nullptr, acc, sweep_bwd::IntegerSum{S});
}

}  // namespace

size_t sweep_backward_det_workspace_bytes(int B, int V, int C, int H, int W) {
    return det_workspace_bytes(B, HDR_WORDS, (size_t)V * C * H * W);
}

hipError_t launch_sweep_backward_det(const SweepArgs& a, const float* grad_cost, float* grad_src, void* workspace, hipStream_t stream) {
    const size_t HW = (size_t)a.H * a.W;
    uint32_t* hdr = static_cast<uint32_t*>(workspace);
    unsigned long long* acc = det_accumulator(workspace, a.B, HDR_WORDS);
    hipError_t e = launch_zero(workspace, sweep_backward_det_workspace_bytes(a.B, a.V, a.C, a.H, a.W), stream);
    if (e != hipSuccess) return e;
    const size_t per_block = 256 * 16;   // (elements a block of the pre-pass reads at least, up to 512 blocks per item and array)
    const size_t want = ((size_t)(a.D > a.C ? a.D : a.C) * HW + per_block - 1) / per_block;
    const unsigned nblk = (unsigned)(want < 512 ? want : 512);
    hipLaunchKernelGGL(sweep_det_bounds_kernel, dim3(nblk, a.B, a.metric == 0 ? 3 : 1), dim3(256), 0, stream, a, grad_cost, hdr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t lds = lds_bytes<sweep_bwd::IntegerSum>(a.D);
    auto go = [&](auto kern) -> hipError_t {
        hipError_t err = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL(kern, grid<sweep_bwd::IntegerSum>(a), dim3(BTHREADS), lds, stream, a, grad_cost, hdr, acc);
        return hipGetLastError();
    };
    e = a.metric == 0 ? go(sweep_bwd_det_kernel<0>) : go(sweep_bwd_det_kernel<1>);
    if (e != hipSuccess) return e;
    return det_convert(workspace, a.B, (size_t)a.V * a.C * HW, ItemExponent(a, a.metric), grad_src, stream);
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entries live here, beside their kernels: capi.o does not refer to this object, so a library
// linked from a subset of the objects still links. ------------------------------------------------------------------------------
extern "C" {

int32_t pdepth_det_scale_exponent(float bound, int64_t n) {
    if (n < 1) return pdepth::fixed::EXP_NONFINITE;
    return pdepth::fixed::det_scale_exponent(bound, n);
}

size_t pdepth_sweep_backward_det_workspace_bytes(const pdepth_sweep_desc* desc) {
    if (!desc || !pdepth::capi::dims_positive(desc)) return 0;
    return pdepth::sweep_backward_det_workspace_bytes(desc->B, desc->V, desc->C, desc->H, desc->W);
}

// est_swp_volume_v4 backward with an order-independent grad_src; grad_ref is the gather pass of sweep_bwd.hip (reproducible as it is)
int pdepth_sweep_backward_det_f32(const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* ref, const float* src,
                                  const float* d_candi, const float* grad_cost, float* grad_ref, float* grad_src, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    using namespace pdepth::capi;
    const char* who = "pdepth_sweep_backward_det_f32";
    if (int rc = check_sweep_backward(who, desc, cam, ref, src, d_candi, grad_cost, grad_ref, grad_src)) return rc;
    if (grad_src) {
        const size_t need = pdepth::sweep_backward_det_workspace_bytes(desc->B, desc->V, desc->C, desc->H, desc->W);
        if (int rc = check_workspace(who, workspace, workspace_bytes, need, "; query pdepth_sweep_backward_det_workspace_bytes()")) return rc;
    }
    pdepth::SweepArgs a = make_args(desc, cam, ref, src, d_candi);
    a.fast_div = 0;
    if (grad_ref) {
        if (int rc = launched(pdepth::launch_sweep_backward(a, grad_cost, grad_ref, nullptr, (hipStream_t)stream), who)) return rc;
    }
    if (!grad_src) return PDEPTH_OK;
    return launched(pdepth::launch_sweep_backward_det(a, grad_cost, grad_src, workspace, (hipStream_t)stream), who);
}

}  // extern "C"
