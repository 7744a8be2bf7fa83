// Evaluation metrics on the device: the KITTI devkit's nine depth errors of a batch of depth maps, without a read-back.
//
// Replaces, per item and per resolution, the tail of DefaultTrainer._validate_with_gt (trainer/default_trainer.py:247-256):
// clamp the ground truth at the last candidate, mask the prediction, copy both maps to the host, img_utils.depth_error
// (utils/img_utils.py:17-22) -> depthError (external/deval_lib/src/evaluate_depth.h:20-121).  Per item b and pixel:
//     p = pred * mask                                (no mask: p = pred)
//     t = truth;  t = clamp_max where t >= clamp_max (clamp_max <= 0: no clamp);  t = -1 where t == 0
//     valid <=> p > 0                                (p == 0 -> -1 -> invalid; a NaN is invalid)
//     over the n valid pixels:  e = |p - t|, ei = |1/p - 1/t|, s = log p - log t, el = |s|
//     mae = S e / n, rmse = sqrt(S e^2 / n), imae = S ei / n, irmse = sqrt(S ei^2 / n), lmae = S el / n,
//     lrmse = sqrt(S el^2 / n), sil = sqrt(S el^2 / n - (S s)^2 / n^2), absrel = S (e / p) / n, sqrel = S (e^2 / p^2) / n
// The argument order of the reference is kept: img_utils.depth_error(predicted, truth) hands its arguments to
// depthError(D_gt, D_ipol) in that order, so validity comes from the masked PREDICTION and the two relative errors divide by the
// PREDICTION.  A valid pixel whose truth is 0 or negative gives NaN (no guard, as in the reference); where the reference throws
// (n == 0) the nine values of that item are NaN and count[b] = 0.
//
// Two forms of the input.  Depth map form: pred [B,H,W], one pixel per thread.  Volume form: logp [B,D,H,W] + d_candi, the
// expectation sum_d d_d exp(logp_d) formed in registers from one read of the volume (4 HW D bytes per item, + 4 HW for the
// truth [+ 4 HW mask] [+ 4 HW for the depth map, written from the same pass]), with the expectation of dpv_lanes.hpp
// (expect_planes): the bits of pdepth_dpv_expect_f32(bv_log = 1).
//
// The volume kernel uses the wave layout of dpv_lanes.hpp.  After the sum over the plane groups every group holds the four
// depths of its quad: lane (g, q) takes pixel 4 q + g of the wave's 64 for the error terms, so each lane evaluates one pixel.
// The other two kernels give lane (g, q) the same pixel (thread_pixel): the three feed the reduction alike, and the metrics of
// the volume form equal those of the depth map form on the map it writes bit for bit.
//
// Pixel reduction: the per-pixel terms are float (as in the reference), their sums double.  Every workgroup (256 pixels) writes
// one record -- the nine sums (the reference's eight error accumulators and its logSum) and the count -- into the workspace; a
// second launch of one workgroup per item adds the records in a fixed order (that of wg_sum_put / wg_sum_get) and finishes the roots.
// No atomics: two calls give the same bits.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "dpv_lanes.hpp"
#include "kernels.hpp"

namespace pdepth {

namespace {

constexpr int NSUM = 9;          // sums of a record: e, e^2, ei, ei^2, el, el^2, s, e/p, e^2/p^2
constexpr int REC = NSUM + 1;    // + the count (a double: exact)

struct MetArgs {
    const float* logp;    // [B,D,H,W] (volume form)
    const float* pred;    // [B,H,W]   (depth map form)
    const float* dc;
    const float* truth;   // [B,H,W]
    const float* mask;    // [B,H,W] or nullptr
    float clamp_max;      // <= 0: no clamp
    int D, HW, nblk;
    float* depth;         // [B,H,W] or nullptr (volume form)
    double* part;         // [B,nblk,REC]
};

// the terms of one pixel (evaluate_depth.h:54-88 with D_gt = the masked prediction, D_ipol = the truth), zeros where invalid
__device__ __forceinline__ void pixel_terms(float pr, int pix, int b, bool live, const MetArgs& a, double (&acc)[REC]) {
#pragma unroll
    for (int j = 0; j < REC; ++j) acc[j] = 0.0;
    if (!live) return;
    const size_t i = (size_t)b * a.HW + pix;
    const float p = a.mask ? pr * a.mask[i] : pr;
    float t = a.truth[i];
    if (a.clamp_max > 0.0f && t >= a.clamp_max) t = a.clamp_max;
    if (t == 0.0f) t = -1.0f;
    if (p > 0.0f) {
        const float e = fabsf(p - t), e2 = e * e;
        const float ei = fabsf(1.0f / p - 1.0f / t);
        const float s = logf(p) - logf(t), el = fabsf(s);
        acc[0] = e; acc[1] = e2; acc[2] = ei; acc[3] = ei * ei; acc[4] = el; acc[5] = el * el; acc[6] = s;
        acc[7] = e / p; acc[8] = e2 / (p * p);
        acc[9] = 1.0;
    }
}

// the record of a workgroup -> its slot of the workspace, in the order of wg_sum_put / wg_sum_get (dpv_lanes.hpp: lanes by
// xor-shuffles 32 ... 1, then (w0 + w1) + (w2 + w3)); written out for the ten sums at once: through the helper, one sum at a
// time, the depth map kernel ran 5 - 7 % slower (profiles/r11_dpv_lanes/README.md)
__device__ __forceinline__ void block_record(double (&acc)[REC], const MetArgs& a, int b) {
    __shared__ double sw[4][REC];
#pragma unroll
    for (int j = 0; j < REC; ++j) {
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) acc[j] = acc[j] + __shfl_xor(acc[j], sh);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < REC; ++j) sw[threadIdx.x >> 6][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < REC) {
        const int j = threadIdx.x;
        a.part[((size_t)b * a.nblk + blockIdx.x) * REC + j] = (sw[0][j] + sw[1][j]) + (sw[2][j] + sw[3][j]);
    }
}

// volume form, H W a multiple of 4 and D <= 4 RPL: CH 16-byte loads in flight per lane
template <int RPL>
__global__ __launch_bounds__(256) void depth_metrics_vec4_kernel(MetArgs a) {
    constexpr int CH = RPL < 16 ? RPL : 16;
    const int D = a.D, HW = a.HW;
    const QuadLane L = quad_lane(D, HW);
    const int g = L.g, b = L.b;
    const bool live = L.live;
    float4 e = splat4(0.f);
#pragma unroll
    for (int c0 = 0; c0 < RPL; c0 += CH) {
        float4 v[CH];
        load_planes(v, a.logp, L, c0, D, HW, 0.f);
        expect_planes<true>(e, v, a.dc, g, c0, D);
    }
    e = group_sum(e);
    const float pr = g == 0 ? e.x : g == 1 ? e.y : g == 2 ? e.z : e.w;   // pixel 4 q + g
    const int pix = L.q * 4 + g;                                          // (= thread_pixel())
    if (a.depth && live) a.depth[(size_t)b * HW + pix] = pr;
    double acc[REC];
    pixel_terms(pr, pix, b, live, a, acc);
    block_record(acc, a, b);
}

// volume form, any D / any H, W / any alignment: one pixel per thread, the planes in a loop (the order of dpv_expect_kernel)
__global__ __launch_bounds__(256) void depth_metrics_scalar_kernel(MetArgs a) {
    const int pix = thread_pixel();
    const bool live = pix < a.HW;
    const int b = blockIdx.y;
    const int D = a.D, HW = a.HW;
    float e = 0.f;
    if (live) {
        const size_t off = (size_t)b * D * HW + pix;
        for (int k = 0; k < D; ++k) e += a.dc[k] * expf(a.logp[off + (size_t)k * HW]);
        if (a.depth) a.depth[(size_t)b * HW + pix] = e;
    }
    double acc[REC];
    pixel_terms(e, pix, b, live, a, acc);
    block_record(acc, a, b);
}

// depth map form
__global__ __launch_bounds__(256) void depth_metrics_map_kernel(MetArgs a) {
    const int pix = thread_pixel();
    const bool live = pix < a.HW;
    const int b = blockIdx.y;
    const float pr = live ? a.pred[(size_t)b * a.HW + pix] : 0.f;
    double acc[REC];
    pixel_terms(pr, pix, b, live, a, acc);
    block_record(acc, a, b);
}

// one workgroup per item: the records in a fixed order -> metrics[b, 0..8], count[b]
__global__ __launch_bounds__(256) void depth_metrics_final_kernel(const double* __restrict__ part, int nblk,
                                                                  float* __restrict__ metrics, float* __restrict__ count) {
    __shared__ double sw[4][REC];
    const int b = blockIdx.x;
    double acc[REC];
#pragma unroll
    for (int j = 0; j < REC; ++j) acc[j] = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) {
#pragma unroll
        for (int j = 0; j < REC; ++j) acc[j] += part[((size_t)b * nblk + i) * REC + j];
    }
#pragma unroll
    for (int j = 0; j < REC; ++j) {   // (the order of block_record)
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) acc[j] = acc[j] + __shfl_xor(acc[j], sh);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < REC; ++j) sw[threadIdx.x >> 6][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double S[REC];
#pragma unroll
        for (int j = 0; j < REC; ++j) S[j] = (sw[0][j] + sw[1][j]) + (sw[2][j] + sw[3][j]);
        const double n = S[9];
        float* m = metrics + (size_t)b * NSUM;
        count[b] = (float)n;
        if (n > 0.0) {
            const double sq_log = S[5] / n;
            m[0] = (float)(S[0] / n);
            m[1] = (float)sqrt(S[1] / n);
            m[2] = (float)(S[2] / n);
            m[3] = (float)sqrt(S[3] / n);
            m[4] = (float)(S[4] / n);
            m[5] = (float)sqrt(sq_log);
            m[6] = (float)sqrt(sq_log - (S[6] * S[6]) / (n * n));
            m[7] = (float)(S[7] / n);
            m[8] = (float)(S[8] / n);
        } else {   // the reference throws here
#pragma unroll
            for (int j = 0; j < NSUM; ++j) m[j] = __builtin_nanf("");
        }
    }
}

}  // namespace

size_t depth_metrics_workspace_bytes(int B, int H, int W) {
    const size_t n = (size_t)B * n_blocks(H, W);
    return (n * REC * sizeof(double) + 255) / 256 * 256;
}

hipError_t launch_depth_metrics(const float* logp, const float* pred, const float* d_candi, const float* truth, const float* mask,
                                float clamp_max, int B, int D, int H, int W, float* metrics, float* count, float* depth,
                                void* workspace, hipStream_t stream) {
    const int HW = H * W, nblk = n_blocks(H, W);
    MetArgs a{};
    a.logp = logp; a.pred = pred; a.dc = d_candi; a.truth = truth; a.mask = mask; a.clamp_max = clamp_max;
    a.D = D; a.HW = HW; a.nblk = nblk; a.depth = depth;
    a.part = static_cast<double*>(workspace);
    const dim3 grid(nblk, B);
    if (pred) {
        hipLaunchKernelGGL(depth_metrics_map_kernel, grid, dim3(256), 0, stream, a);
    } else if ((HW % 4 == 0) && D <= 128 && aligned16(logp) && (!depth || aligned16(depth))) {   // (as launch_dpv_expect decides)
        for_planes_per_lane(D, [&](auto rpl) {
            hipLaunchKernelGGL(depth_metrics_vec4_kernel<decltype(rpl)::value>, grid, dim3(256), 0, stream, a);
        });
    } else {
        hipLaunchKernelGGL(depth_metrics_scalar_kernel, grid, dim3(256), 0, stream, a);
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(depth_metrics_final_kernel, dim3(B), dim3(256), 0, stream, a.part, nblk, metrics, count);
    return hipGetLastError();
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entries live here, beside their kernels: capi.o does not refer to this object, so a
// library linked from a subset of the objects (tests/test_sweep_prefetch.py) still links. ------------------------------------
using namespace pdepth::capi;

extern "C" {

size_t pdepth_depth_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return (B > 0 && H > 0 && W > 0 && (long long)H * W <= (1ll << 30)) ? pdepth::depth_metrics_workspace_bytes(B, H, W) : 0;
}

int pdepth_depth_metrics_f32(const float* logp, const float* pred, const float* d_candi, const float* truth, const float* mask,
                             float clamp_max, int32_t B, int32_t D, int32_t H, int32_t W, float* metrics, float* count,
                             float* depth, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pdepth_depth_metrics_f32";
    if (!truth) return fail(PDEPTH_E_ARG, "%s: null pointer (truth)", who);
    if ((logp != nullptr) == (pred != nullptr))
        return fail(PDEPTH_E_ARG, "%s: exactly one prediction (logp or pred) must be given", who);
    if (logp && !d_candi) return fail(PDEPTH_E_ARG, "%s: null pointer (d_candi): the volume form needs the depth candidates", who);
    if (int rc = check_dims(who, B, logp ? D : 1, H, W)) return rc;   // (D belongs to the volume form)
    if (int rc = check_launch_limits(who, B, H, W)) return rc;
    if (!metrics || !count) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (pred && depth) return fail(PDEPTH_E_ARG, "%s: the depth output belongs to the volume form", who);
    if (int rc = check_workspace(who, workspace, workspace_bytes, pdepth::depth_metrics_workspace_bytes(B, H, W))) return rc;
    return launched(pdepth::launch_depth_metrics(logp, pred, d_candi, truth, mask, clamp_max, B, D, H, W, metrics, count, depth,
                                                 workspace, (hipStream_t)stream), who);
}

}  // extern "C"
