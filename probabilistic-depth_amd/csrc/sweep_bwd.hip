// Backward of the plane sweep with respect to the feature maps: g_cost [B,D,H,W] -> g_ref [B,C,H,W], g_src [B,V,C,H,W].
//
// Differentiates est_swp_volume_v4 (warping/homography.py:98-135: grid_sample bilinear / zeros / align_corners=False,
// :170-198, then img_dis_L2_pard / img_dis_L1_pard :80-86 and the division by sigma).  With w_v the bilinear warp of view v
// into plane k at pixel p and e = w_v(src_v)[c] - ref[c]:
//     L2: g_ref[c,p] = -(2/sigma) sum_v sum_k g[k,p] e,   tap t of (v,k,p) receives (2/sigma) g[k,p] w_t e in g_src[v,c,t]
//     L1: the same with 2e replaced by sign(e), sign(0) = 0 (torch.abs backward)
// Taps outside the image receive nothing (ATen's grid_sampler_2d backward).  Sample positions and bilinear weights come from
// the helpers the gather kernel uses (geometry.hpp plane_sample_pos / make_footprint, sweep_direct.hip), evaluated in plain
// fp32 on the NCHW features: no distance form, no fp16 pairs, no routing.
//
// One workgroup owns a 16 x 16 tile of reference pixels of one batch item and BCC channels (grid z), every view and every
// plane.  The two outputs are two instantiations, launched one after the other when both are requested
// (one kernel for both did not fit the scalar register file):
//   * g_ref is a per-pixel gather kept in registers (summed in double over the planes of a view) and written by the thread that owns the pixel (view after view, read back
//     and added in view order): no atomics, bitwise reproducible from call to call;
//   * g_src is a scatter.  Per view the workgroup first reduces, plane by plane, the bounding box of the in-bounds taps of its
//     tile (LDS).  Consecutive planes are grouped while the union of their boxes fits BOX_CAP texels; a group's taps are summed
//     in an LDS image of the box, kept in double (ds_add_f64), which is then rounded once and added to g_src with global_atomic_add_f32, row-contiguous (the
//     lanes of a wave cover consecutive texels of a box row).  A plane whose box alone does not fit (degenerate geometry,
//     near planes of wide baselines) adds its taps to g_src directly: correct, slower.  The launcher zeroes g_src on the
//     stream first.  The sums of g_src depend on the order in which the adds arrive: results may differ in the last bits
//     from call to call.
// The body of the kernel is sweep_bwd_body.hpp, shared with sweep_bwd_det.hip; here it runs with the policies NoScatter (g_ref) and
// FloatAtomics (g_src: a double box image, float atomicAdd into g_src, 4 channels per pass).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.hpp"
#include "sweep_bwd_body.hpp"

namespace pdepth {

namespace {

using namespace sweep_bwd;

template <int METRIC, bool GREF, bool GSRC>   // GREF / GSRC: the outputs requested (gref / gsrc are not null)
__global__ __launch_bounds__(BTHREADS) void sweep_bwd_kernel(SweepArgs a, const float* __restrict__ gcost,
                                                             float* __restrict__ gref, float* __restrict__ gsrc) {
    sweep_bwd_body<METRIC, GREF>(a, gcost, gref, gsrc, std::conditional_t<GSRC, FloatAtomics, NoScatter>{});
}

}  // namespace

hipError_t launch_sweep_backward(const SweepArgs& a, const float* grad_cost, float* grad_ref, float* grad_src, hipStream_t stream) {
    const size_t HW = (size_t)a.H * a.W;
    if (grad_src) {
        hipError_t e = launch_zero(grad_src, (size_t)a.B * a.V * a.C * HW * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    auto go = [&](auto kern, auto policy) -> hipError_t {
        using Policy = decltype(policy);
        const size_t lds = lds_bytes<Policy>(a.D);
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid<Policy>(a), dim3(BTHREADS), lds, stream, a, grad_cost, grad_ref, grad_src);
        return hipGetLastError();
    };
    // both outputs: two launches (the gather pass is cheap beside the scatter; one kernel for both did not fit the scalar file)
    hipError_t e = hipSuccess;
    if (grad_ref) e = a.metric == 0 ? go(sweep_bwd_kernel<0, true, false>, NoScatter{}) : go(sweep_bwd_kernel<1, true, false>, NoScatter{});
    if (e == hipSuccess && grad_src)
        e = a.metric == 0 ? go(sweep_bwd_kernel<0, false, true>, FloatAtomics{}) : go(sweep_bwd_kernel<1, false, true>, FloatAtomics{});
    return e;
}

}  // namespace pdepth
