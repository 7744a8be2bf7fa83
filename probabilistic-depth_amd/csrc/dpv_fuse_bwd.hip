// Backward of the DPV Bayesian fusion (dpv_fuse.hip) with respect to the incoming log-DPV -- what autograd does behind
// models/models.py:666-672 for BV_cur; the depth map, the mask and the candidates are data.
//
// Per pixel, x_k the incoming log-DPV (not necessarily normalised):
//     m_k  = the prior the forward builds (Gaussian of d_k - dmap normalised over k, NaN -> -1, blended with the uniform DPV
//            by the mask, clamp(eps, 1)) -- constant with respect to x
//     u_k  = exp(x_k + log m_k),  S = sum_k u_k,  q_k = u_k / S
//     forward outputs: fused_k = clamp(q_k, eps, 1), log_fused_k = log fused_k
// With g_f into fused and g_l into log_fused (either may be absent):
//     c_k   = pass_k (g_f,k q_k + g_l,k),   pass_k = (eps <= q_k <= 1)   (torch.clamp's rule; on a passing plane fused = q, so
//             g_l / fused * q = g_l: no division by eps)
//     T     = sum_k c_k
//     g_x,k = c_k - q_k T                   (clamped planes too: c_k = 0, but they still receive -q_k T)
// m and q are recomputed from logp, dmaps and masks with the forward's own operations (dpv_fuse_math.hpp), so pass_k is decided
// on the value the forward clamped; nothing but the inputs is saved.  Lane = pixel, no atomics, no cross-lane traffic: the
// result is reproducible bit for bit, and a non-finite value stays inside its pixel's column.
// Traffic, V = 4 B D H W, P = 4 B H W bytes: reads V (1 + number of gradients present) + 2 P, writes V.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "dpv_fuse_math.hpp"
#include "kernels.hpp"

namespace pdepth {

namespace {

// D <= DREG: the column lives in registers between the sweeps over k like in dpv_fuse_reg_kernel (x, then u in its place;
// the Gaussian; one gradient, then c in its place), so logp, g_f and g_l are read once and g_x is written once.  With both
// gradients present g_l is loaded into the Gaussian's registers once the second sweep has released them -- a fourth array of
// DREG floats would not fit 256 registers.  FULL: D == DREG, no plane is skipped and the whole kernel is one basic block.

// a copy of the (uniform) plane count that the compiler cannot identify with another one
__device__ __forceinline__ int planes_of(int D) {
    asm volatile("" : "+s"(D));
    return D;
}

template <int DREG, bool FULL, bool HAS_F, bool HAS_L>
__global__ __launch_bounds__(256) void dpv_fuse_bwd_reg_kernel(const float* __restrict__ logp, const float* __restrict__ dmaps,
                                                               const float* __restrict__ masks, const float* __restrict__ dc,
                                                               const float* __restrict__ g_fused,
                                                               const float* __restrict__ g_logfused, int D, int HW, float var,
                                                               float eps, float* __restrict__ g_logp) {
    static_assert(HAS_F || HAS_L, "at least one incoming gradient");
    __shared__ float s_dc[DREG];
    for (int k = threadIdx.x; k < DREG; k += 256) s_dc[k] = k < D ? dc[k] : 0.0f;
    __syncthreads();
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const float dmap = dmaps[(size_t)b * HW + pix];
    const float mask = masks[(size_t)b * HW + pix];
    const float inv_mask = 1.0f - mask;
    const float sigma = sqrtf(var);
    const float two_var = 2.0f * (sigma * sigma);  // 2 * torch.pow(sig, 2)
    const float r_two_var = fuse_rcp(two_var);
    const float uni = 1.0f / (float)D;
    const size_t col = (size_t)b * D * HW + pix;
    const float* lp = logp + col;
    const float* gf = HAS_F ? g_fused + col : nullptr;
    const float* gl = HAS_L ? g_logfused + col : nullptr;
    float v[DREG], x[DREG], c[DREG];
    // Planes beyond D are skipped by uniform branches (!FULL).  Each sweep compares k with a copy of D of its own (planes_of): compared
    // with the one D, the DREG predicates are kept as lane masks from the first sweep to the last and do not fit the SGPR file.
    // Each stream walks its column with a pointer of its own for the same reason (no DREG plane offsets k * HW).
    const int D1 = planes_of(D);
#pragma unroll
    for (int k = 0; k < DREG; ++k, lp += HW) {
        if (FULL || k < D1) {
            x[k] = __builtin_nontemporal_load(lp);
        }
    }
    const float* g1 = HAS_F ? gf : gl;
    const int D2 = planes_of(D);
#pragma unroll
    for (int k = 0; k < DREG; ++k, g1 += HW) {
        if (FULL || k < D2) {
            c[k] = __builtin_nontemporal_load(g1);
        }
    }
    // the forward's first two sweeps, operation for operation
    float sumg = 0.0f;
    const int D3 = planes_of(D);
#pragma unroll
    for (int k = 0; k < DREG; ++k) {
        if (FULL || k < D3) {
            const float a = fabsf(s_dc[k] - dmap);
            v[k] = fuse_exp(fuse_div(-(a * a), two_var, r_two_var));
            sumg = sumg + v[k];
        }
    }
    float sumf = 0.0f;
    const float r_sumg = fuse_rcp(sumg);
    const int D4 = planes_of(D);
#pragma unroll
    for (int k = 0; k < DREG; ++k) {
        if (FULL || k < D4) {
            float t = fuse_div(v[k], sumg, r_sumg);
            if (t != t) t = -1.0f;                       // zero_invalid (img_utils.py:45)
            const float m = t * mask + uni * inv_mask;   // img_utils.py:371
            x[k] = fuse_exp(x[k] + fuse_log(fminf(fmaxf(m, eps), 1.0f)));
            sumf = sumf + x[k];
        }
    }
    if (HAS_F && HAS_L) {   // the second gradient, into the registers the Gaussian has left: issued back to back, one wait
        const int D7 = planes_of(D);
#pragma unroll
        for (int k = 0; k < DREG; ++k, gl += HW) {
            if (FULL || k < D7) {
                v[k] = __builtin_nontemporal_load(gl);
            }
        }
    }
    const float r_sumf = fuse_rcp(sumf);
    float T = 0.0f;
    const int D5 = planes_of(D);
#pragma unroll
    for (int k = 0; k < DREG; ++k) {
        if (FULL || k < D5) {
            const float q = fuse_div(x[k], sumf, r_sumf);   // what the forward clamps
            x[k] = q;
            float g = HAS_F ? c[k] * q : c[k];
            if (HAS_F && HAS_L) g = g + v[k];
            c[k] = (q >= eps && q <= 1.0f) ? g : 0.0f;      // (a NaN q does not pass)
            T = T + c[k];
        }
    }
    float* o = g_logp + col;
    const int D6 = planes_of(D);
#pragma unroll
    for (int k = 0; k < DREG; ++k, o += HW) {
        if (FULL || k < D6) {
            __builtin_nontemporal_store(c[k] - x[k] * T, o);
        }
    }
}

// Any D: the columns are re-read (from L2) in the later sweeps, like dpv_fuse_kernel.  FAST: the arithmetic of
// dpv_fuse_reg_kernel (what the forward runs up to 128 planes); otherwise libm's, as in dpv_fuse_kernel.  An absent gradient
// is a uniform branch: no loads.
template <bool FAST>
__global__ __launch_bounds__(256) void dpv_fuse_bwd_kernel(const float* __restrict__ logp, const float* __restrict__ dmaps,
                                                           const float* __restrict__ masks, const float* __restrict__ dc,
                                                           const float* __restrict__ g_fused, const float* __restrict__ g_logfused,
                                                           int D, int HW, float var, float eps, float* __restrict__ g_logp) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int b = blockIdx.y;
    const float dmap = dmaps[(size_t)b * HW + pix];
    const float mask = masks[(size_t)b * HW + pix];
    const float inv_mask = 1.0f - mask;
    const float sigma = sqrtf(var);
    const float two_var = 2.0f * (sigma * sigma);  // 2 * torch.pow(sig, 2)
    const float r_two_var = FAST ? fuse_rcp(two_var) : 0.0f;
    const float uni = 1.0f / (float)D;
    const size_t col = (size_t)b * D * HW + pix;
    const float* lp = logp + col;
    auto gauss = [&](int k) {
        const float a = fabsf(dc[k] - dmap);
        return FAST ? fuse_exp(fuse_div(-(a * a), two_var, r_two_var)) : expf(-(a * a) / two_var);
    };
    float sumg = 0.0f;
    for (int k = 0; k < D; ++k) sumg = sumg + gauss(k);
    const float r_sumg = FAST ? fuse_rcp(sumg) : 0.0f;
    auto unnorm = [&](int k) {   // u_k
        float t = FAST ? fuse_div(gauss(k), sumg, r_sumg) : gauss(k) / sumg;
        if (t != t) t = -1.0f;                       // zero_invalid (img_utils.py:45)
        const float m = fminf(fmaxf(t * mask + uni * inv_mask, eps), 1.0f);   // img_utils.py:371
        const float xk = lp[(size_t)k * HW];
        return FAST ? fuse_exp(xk + fuse_log(m)) : expf(xk + logf(m));
    };
    float sumf = 0.0f;
    for (int k = 0; k < D; ++k) sumf = sumf + unnorm(k);
    const float r_sumf = FAST ? fuse_rcp(sumf) : 0.0f;
    auto passed = [&](int k, float q) {   // c_k
        const size_t i = col + (size_t)k * HW;
        float g = g_fused ? g_fused[i] * q : 0.0f;
        if (g_logfused) g = g_fused ? g + g_logfused[i] : g_logfused[i];
        return (q >= eps && q <= 1.0f) ? g : 0.0f;
    };
    float T = 0.0f;
    for (int k = 0; k < D; ++k) {
        const float q = FAST ? fuse_div(unnorm(k), sumf, r_sumf) : unnorm(k) / sumf;
        T = T + passed(k, q);
    }
    for (int k = 0; k < D; ++k) {
        const float q = FAST ? fuse_div(unnorm(k), sumf, r_sumf) : unnorm(k) / sumf;
        g_logp[col + (size_t)k * HW] = passed(k, q) - q * T;
    }
}

}  // namespace

hipError_t launch_dpv_fuse_backward(const float* logp, const float* dmaps, const float* masks, const float* d_candi,
                                    const float* g_fused, const float* g_logfused, int B, int D, int H, int W, float var, float eps,
                                    float* g_logp, hipStream_t stream) {
    if (!g_fused && !g_logfused) return hipErrorInvalidValue;
    const int HW = H * W;
    dim3 grid((HW + 255) / 256, B);
#define PDEPTH_FUSE_BWD(kern) \
    hipLaunchKernelGGL((kern), grid, dim3(256), 0, stream, logp, dmaps, masks, d_candi, g_fused, g_logfused, D, HW, var, eps, g_logp)
    if (D <= 64) {
        const int which = (g_fused ? 2 : 0) + (g_logfused ? 1 : 0);
        if (D == 64) {
            if (which == 3) PDEPTH_FUSE_BWD((dpv_fuse_bwd_reg_kernel<64, true, true, true>));
            else if (which == 2) PDEPTH_FUSE_BWD((dpv_fuse_bwd_reg_kernel<64, true, true, false>));
            else PDEPTH_FUSE_BWD((dpv_fuse_bwd_reg_kernel<64, true, false, true>));
        } else {
            if (which == 3) PDEPTH_FUSE_BWD((dpv_fuse_bwd_reg_kernel<64, false, true, true>));
            else if (which == 2) PDEPTH_FUSE_BWD((dpv_fuse_bwd_reg_kernel<64, false, true, false>));
            else PDEPTH_FUSE_BWD((dpv_fuse_bwd_reg_kernel<64, false, false, true>));
        }
    } else if (D <= 128) {   // (the forward's 128-plane register kernel; a backward of that form needs more than 256 registers)
        PDEPTH_FUSE_BWD(dpv_fuse_bwd_kernel<true>);
    } else {
        PDEPTH_FUSE_BWD(dpv_fuse_bwd_kernel<false>);
    }
#undef PDEPTH_FUSE_BWD
    return hipGetLastError();
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entry lives here, beside its kernels, like those of loss.hip and metrics.hip: capi.o does
// not refer to this object, so a library linked from a subset of the objects (tests/test_sweep_prefetch.py) still links. ----
using namespace pdepth::capi;

extern "C" {

// DPV fusion backward with respect to the log-DPV (models/models.py:666-672; the prior of utils/img_utils.py:360-375 is data)
int pdepth_dpv_fuse_backward_f32(const float* logp, const float* dmaps, const float* masks, const float* d_candi,
                                 const float* g_fused, const float* g_logfused, int32_t B, int32_t D, int32_t H, int32_t W,
                                 float var, float eps, float* g_logp, void* stream) {
    const char* who = "pdepth_dpv_fuse_backward_f32";
    if (!logp || !dmaps || !masks || !d_candi || !g_logp) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!g_fused && !g_logfused) return fail(PDEPTH_E_ARG, "%s: no incoming gradient", who);
    if (int rc = check_dims(who, B, D, H, W)) return rc;
    if (int rc = check_launch_limits(who, B, H, W)) return rc;
    if (!(var > 0.0f)) return fail(PDEPTH_E_ARG, "%s: var must be positive", who);
    if ((const float*)g_logp == logp || (const float*)g_logp == g_fused || (const float*)g_logp == g_logfused)
        return fail(PDEPTH_E_ARG, "%s: g_logp may not alias an input", who);
    return launched(pdepth::launch_dpv_fuse_backward(logp, dmaps, masks, d_candi, g_fused, g_logfused, B, D, H, W, var, eps, g_logp,
                                                     (hipStream_t)stream), who);
}

}  // extern "C"
