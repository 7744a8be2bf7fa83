// Training loss on a log-DPV: soft-label cross-entropy over the depth axis (+ the expectation), forward and backward.
//
// Replaces soft_cross_entropy_loss(BV_log=True) (losses/loss_blocks.py:186-202) called per item and per side by BaseLoss
// (losses/losses.py:32-67), the dpv_to_depthmap that follows on the same volume (losses/losses.py:80-88;
// utils/img_utils.py:52-61) and, in the from-depth form, gen_soft_label_torch(zero_invalid=True) (utils/img_utils.py:24-47;
// kittiloader/batch_scheduler.py:99-109).  Per item b and pixel p:
//     ce[b,p]   = - sum_d label[b,d,p] logp[b,d,p]
//     loss[b]   = sum_p ce[b,p] mask[b,p] / count[b],  count[b] = #{p : mask[b,p] == 1}   (0 where count[b] == 0;
//                 the mean over all pixels without a mask)
//     depth[b,p]= sum_d d_d exp(logp[b,d,p])                                                (optional)
// The label is read ([B,D,H,W]) or formed from a depth map: g_d = exp(-|d_d - z|^pow / (2 sqrt(variance)^pow)),
// label_d = g_d / sum_d g_d, -1 on every plane where the sum is 0 or NaN.  In that form no label is stored anywhere: the
// forward needs sum_d g_d logp_d and sum_d g_d only, ce = -(sum_d g_d logp_d) / (sum_d g_d).
//
// Bytes per volume: forward 4 HW (D + 1 [+ D with a label tensor] [+ 1 mask] [+ 1 depth]); backward 4 HW D written once
// (+ 4 HW D for the label tensor, + 4 HW D for logp when a depth gradient comes in).  The reference's composition reads or
// writes [D,H,W] ten times forward.
//
// The vec4 kernels use the wave layout of dpv_lanes.hpp and its expectation (expect_add: the bits of pdepth_dpv_expect_f32).
// The loads are issued CH planes at a time (the volume and the label: 2 CH 16-byte loads in flight per lane).
//
// Pixel reduction: every workgroup (256 pixels) writes one partial sum and one count into the workspace, a second launch
// of one workgroup per item adds them in a fixed order (wg_sum_put / wg_sum_get).  No atomics: two calls give the same bits.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "dpv_lanes.hpp"
#include "kernels.hpp"

namespace pdepth {

namespace {

struct Gauss {   // gaussian_torch (utils/img_utils.py:24-25) with sig = sqrt(variance)
    float den;   // 2 sig^pow
    float pw;
    int square;  // pow == 2: |x|^2 as a product, like torch.pow(x, 2.)
    __device__ __forceinline__ float operator()(float dk, float z) const {
        const float a = fabsf(dk - z);
        const float p = square ? a * a : powf(a, pw);
        return expf(-p / den);
    }
};

struct CeArgs {
    const float* logp;
    const float* dc;
    const float* label;     // [B,D,H,W] or nullptr
    const float* depth_gt;  // [B,H,W] or nullptr
    const float* mask;      // [B,H,W] or nullptr
    Gauss gs;
    int D, HW, nblk;
    float* depth;           // [B,H,W] or nullptr
    float* part_sum;        // [B,nblk]
    int* part_cnt;          // [B,nblk]
};

constexpr int CH = 8;   // planes of a lane in flight together

// sum and count of a workgroup -> its slot of the workspace
__device__ __forceinline__ void block_partial(float w, int c, const CeArgs& a, int b) {
    __shared__ float sw[4];
    __shared__ int sc[4];
    wg_sum_put(w, sw);
    wg_sum_put(c, sc);
    __syncthreads();
    if (threadIdx.x == 0) {
        a.part_sum[(size_t)b * a.nblk + blockIdx.x] = wg_sum_get(sw);
        a.part_cnt[(size_t)b * a.nblk + blockIdx.x] = wg_sum_get(sc);
    }
}

// weight of a pixel: masked-out pixels are skipped, not multiplied (a -inf or NaN behind a zero mask stays there)
__device__ __forceinline__ void weigh(float ce, float m, float& w, int& c) {
    if (m != 0.0f) w += ce * m;
    c += (m == 1.0f) ? 1 : 0;
}

template <bool FROM_DEPTH, int RPL>
__global__ __launch_bounds__(256) void soft_ce_vec4_kernel(CeArgs a) {
    const int D = a.D, HW = a.HW;
    const QuadLane L = quad_lane(D, HW);
    const int g = L.g, b = L.b;
    const bool live = L.live;
    const float4 zero = splat4(0.f);
    float4 z = zero;
    if (FROM_DEPTH) z = load_quad(a.depth_gt, L, 0.f);
    const bool want_depth = a.depth != nullptr;
    float4 e = zero, num = zero, S = zero, slp = zero;
#pragma unroll
    for (int c0 = 0; c0 < RPL; c0 += CH) {
        float4 v[CH], l[CH];
        load_planes(v, a.logp, L, c0, D, HW, 0.f);
        if (!FROM_DEPTH) load_planes(l, a.label, L, c0, D, HW, 0.f);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int k = g + 4 * (c0 + u);
            if (k < D) {
                const float dk = a.dc[k];
                if (want_depth) expect_add<true>(e, dk, v[u]);
                if (FROM_DEPTH) {
                    const float4 w = make_float4(a.gs(dk, z.x), a.gs(dk, z.y), a.gs(dk, z.z), a.gs(dk, z.w));
                    S.x += w.x; S.y += w.y; S.z += w.z; S.w += w.w;
                    num.x += w.x * v[u].x; num.y += w.y * v[u].y; num.z += w.z * v[u].z; num.w += w.w * v[u].w;
                    slp.x += v[u].x; slp.y += v[u].y; slp.z += v[u].z; slp.w += v[u].w;
                } else {
                    num.x += l[u].x * v[u].x; num.y += l[u].y * v[u].y;
                    num.z += l[u].z * v[u].z; num.w += l[u].w * v[u].w;
                }
            }
        }
    }
    num = group_sum(num);
    float4 ce = make_float4(-num.x, -num.y, -num.z, -num.w);
    if (FROM_DEPTH) {
        S = group_sum(S);
        slp = group_sum(slp);
        // sum 0 or NaN: the label is -1 on every plane (zero_invalid), ce = sum_d logp_d
        ce.x = S.x > 0.0f ? -(num.x / S.x) : slp.x; ce.y = S.y > 0.0f ? -(num.y / S.y) : slp.y;
        ce.z = S.z > 0.0f ? -(num.z / S.z) : slp.z; ce.w = S.w > 0.0f ? -(num.w / S.w) : slp.w;
    }
    if (want_depth) {
        e = group_sum(e);
        if (live && g == 0) *reinterpret_cast<float4*>(a.depth + L.poff) = e;
    }
    float w = 0.0f;
    int cnt = 0;
    if (live && g == 0) {
        const float4 m = a.mask ? *reinterpret_cast<const float4*>(a.mask + L.poff) : splat4(1.f);
        float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
        weigh(ce.x, m.x, w0, cnt); weigh(ce.y, m.y, w1, cnt); weigh(ce.z, m.z, w2, cnt); weigh(ce.w, m.w, w3, cnt);
        w = (w0 + w1) + (w2 + w3);
    }
    block_partial(w, cnt, a, b);
}

// any D / any H, W / any alignment: one pixel per thread, the planes in a loop (the order of dpv_expect_kernel)
template <bool FROM_DEPTH>
__global__ __launch_bounds__(256) void soft_ce_scalar_kernel(CeArgs a) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const bool live = pix < a.HW;
    const int b = blockIdx.y;
    const int D = a.D, HW = a.HW;
    float w = 0.0f;
    int cnt = 0;
    if (live) {
        const size_t off = (size_t)b * D * HW + pix;
        const float m = a.mask ? a.mask[(size_t)b * HW + pix] : 1.0f;
        const float z = FROM_DEPTH ? a.depth_gt[(size_t)b * HW + pix] : 0.0f;
        float e = 0.f, num = 0.f, S = 0.f, slp = 0.f;
        for (int k = 0; k < D; ++k) {
            const float v = a.logp[off + (size_t)k * HW];
            const float dk = a.dc[k];
            if (a.depth) e += dk * expf(v);
            if (FROM_DEPTH) {
                const float gk = a.gs(dk, z);
                S += gk;
                num += gk * v;
                slp += v;
            } else {
                num += a.label[off + (size_t)k * HW] * v;
            }
        }
        float ce = -num;
        if (FROM_DEPTH) ce = S > 0.0f ? -(num / S) : slp;
        if (a.depth) a.depth[(size_t)b * HW + pix] = e;
        weigh(ce, m, w, cnt);
    }
    block_partial(w, cnt, a, b);
}

// one workgroup per item: the partial sums in a fixed order -> loss[b], count[b]
__global__ __launch_bounds__(256) void soft_ce_final_kernel(const float* __restrict__ part_sum, const int* __restrict__ part_cnt,
                                                            int nblk, int HW, int has_mask, float* __restrict__ loss,
                                                            float* __restrict__ count) {
    __shared__ double ss[4];
    __shared__ long long sc[4];
    const int b = blockIdx.x;
    double s = 0.0;
    long long c = 0;
    for (int i = threadIdx.x; i < nblk; i += 256) {
        s += (double)part_sum[(size_t)b * nblk + i];
        c += part_cnt[(size_t)b * nblk + i];
    }
    wg_sum_put(s, ss);
    wg_sum_put(c, sc);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tot = wg_sum_get(ss);
        const float n = has_mask ? (float)wg_sum_get(sc) : (float)HW;
        count[b] = n;
        loss[b] = n > 0.0f ? (float)tot / n : 0.0f;
    }
}

struct CeBwdArgs {
    const float* logp;
    const float* dc;
    const float* label;
    const float* depth_gt;
    const float* mask;
    const float* count;    // [B], from the forward
    const float* g_loss;   // [B] or nullptr (zero)
    const float* g_depth;  // [B,H,W] or nullptr (zero)
    Gauss gs;
    int D, HW;
    float* g_logp;
};

// - g_loss[b] mask / count[b]: 0 for an item without a valid pixel and for a masked-out pixel
__device__ __forceinline__ float pixel_coef(float gl, float n, float m) {
    return (n > 0.0f && m != 0.0f) ? -(gl * m / n) : 0.0f;
}

template <bool FROM_DEPTH, int RPL>
__global__ __launch_bounds__(256) void soft_ce_bwd_vec4_kernel(CeBwdArgs a) {
    const int D = a.D, HW = a.HW;
    const QuadLane L = quad_lane(D, HW);
    const int g = L.g, b = L.b;
    const bool live = L.live;
    const float4 zero = splat4(0.f);
    const float gl = a.g_loss ? a.g_loss[b] : 0.0f;
    const float n = a.count[b];
    const float4 m = a.mask ? load_quad(a.mask, L, 1.f) : splat4(1.f);
    const float4 c = make_float4(pixel_coef(gl, n, m.x), pixel_coef(gl, n, m.y), pixel_coef(gl, n, m.z), pixel_coef(gl, n, m.w));
    const bool have_gd = a.g_depth != nullptr;
    const float4 gd = have_gd ? load_quad(a.g_depth, L, 0.f) : zero;
    float4 z = zero, S = zero;
    if (FROM_DEPTH) {
        z = load_quad(a.depth_gt, L, 0.f);
#pragma unroll
        for (int i = 0; i < RPL; ++i) {
            const int k = g + 4 * i;
            if (k < D) {
                const float dk = a.dc[k];
                S.x += a.gs(dk, z.x); S.y += a.gs(dk, z.y); S.z += a.gs(dk, z.z); S.w += a.gs(dk, z.w);
            }
        }
        S = group_sum(S);
    }
#pragma unroll
    for (int c0 = 0; c0 < RPL; c0 += CH) {
        float4 v[CH], l[CH];
        load_planes(v, a.logp, L, c0, D, HW, 0.f, have_gd);
        if (!FROM_DEPTH) load_planes(l, a.label, L, c0, D, HW, 0.f);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int k = g + 4 * (c0 + u);
            if (k < D && live) {
                const float dk = a.dc[k];
                float4 lab;
                if (FROM_DEPTH) {
                    lab.x = S.x > 0.0f ? a.gs(dk, z.x) / S.x : -1.0f; lab.y = S.y > 0.0f ? a.gs(dk, z.y) / S.y : -1.0f;
                    lab.z = S.z > 0.0f ? a.gs(dk, z.z) / S.z : -1.0f; lab.w = S.w > 0.0f ? a.gs(dk, z.w) / S.w : -1.0f;
                } else {
                    lab = l[u];
                }
                float4 o = make_float4(c.x != 0.0f ? c.x * lab.x : 0.0f, c.y != 0.0f ? c.y * lab.y : 0.0f,
                                       c.z != 0.0f ? c.z * lab.z : 0.0f, c.w != 0.0f ? c.w * lab.w : 0.0f);
                if (have_gd) {
                    o.x += (gd.x * dk) * expf(v[u].x); o.y += (gd.y * dk) * expf(v[u].y);
                    o.z += (gd.z * dk) * expf(v[u].z); o.w += (gd.w * dk) * expf(v[u].w);
                }
                store_nt(a.g_logp + L.off + (size_t)k * HW, o);
            }
        }
    }
}

template <bool FROM_DEPTH>
__global__ __launch_bounds__(256) void soft_ce_bwd_scalar_kernel(CeBwdArgs a) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= a.HW) return;
    const int b = blockIdx.y;
    const int D = a.D, HW = a.HW;
    const size_t off = (size_t)b * D * HW + pix;
    const float m = a.mask ? a.mask[(size_t)b * HW + pix] : 1.0f;
    const float c = pixel_coef(a.g_loss ? a.g_loss[b] : 0.0f, a.count[b], m);
    const float gd = a.g_depth ? a.g_depth[(size_t)b * HW + pix] : 0.0f;
    const float z = FROM_DEPTH ? a.depth_gt[(size_t)b * HW + pix] : 0.0f;
    float S = 0.0f;
    if (FROM_DEPTH)
        for (int k = 0; k < D; ++k) S += a.gs(a.dc[k], z);
    for (int k = 0; k < D; ++k) {
        const size_t i = off + (size_t)k * HW;
        const float dk = a.dc[k];
        const float lab = FROM_DEPTH ? (S > 0.0f ? a.gs(dk, z) / S : -1.0f) : a.label[i];
        float o = c != 0.0f ? c * lab : 0.0f;
        if (a.g_depth) o += (gd * dk) * expf(a.logp[i]);
        a.g_logp[i] = o;
    }
}

Gauss make_gauss(float variance, float pw) {
    Gauss gs;
    const float sig = sqrtf(variance);
    gs.square = pw == 2.0f;
    gs.pw = pw;
    gs.den = 2.0f * (gs.square ? sig * sig : powf(sig, pw));
    return gs;
}

}  // namespace

size_t dpv_soft_ce_workspace_bytes(int B, int H, int W) {
    const size_t n = (size_t)B * n_blocks(H, W);
    return (n * (sizeof(float) + sizeof(int)) + 255) / 256 * 256;
}

hipError_t launch_dpv_soft_ce(const float* logp, const float* d_candi, const float* label, const float* depth_gt, float variance,
                              float pw, const float* mask, int B, int D, int H, int W, float* loss, float* count, float* depth,
                              void* workspace, hipStream_t stream) {
    const int HW = H * W, nblk = n_blocks(H, W);
    CeArgs a{};
    a.logp = logp; a.dc = d_candi; a.label = label; a.depth_gt = depth_gt; a.mask = mask;
    if (depth_gt) a.gs = make_gauss(variance, pw);
    a.D = D; a.HW = HW; a.nblk = nblk; a.depth = depth;
    a.part_sum = static_cast<float*>(workspace);
    a.part_cnt = reinterpret_cast<int*>(a.part_sum + (size_t)B * nblk);
    const bool vec = (HW % 4 == 0) && D <= 128 && aligned16(logp) && (!label || aligned16(label)) &&
                     (!depth_gt || aligned16(depth_gt)) && (!mask || aligned16(mask)) && (!depth || aligned16(depth));
    const dim3 grid(nblk, B);
    if (vec) {
        for_planes_per_lane(D, [&](auto rpl) {
            constexpr int RPL = decltype(rpl)::value;
            if (depth_gt) hipLaunchKernelGGL((soft_ce_vec4_kernel<true, RPL>), grid, dim3(256), 0, stream, a);
            else hipLaunchKernelGGL((soft_ce_vec4_kernel<false, RPL>), grid, dim3(256), 0, stream, a);
        });
    } else if (depth_gt) {
        hipLaunchKernelGGL(soft_ce_scalar_kernel<true>, grid, dim3(256), 0, stream, a);
    } else {
        hipLaunchKernelGGL(soft_ce_scalar_kernel<false>, grid, dim3(256), 0, stream, a);
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(soft_ce_final_kernel, dim3(B), dim3(256), 0, stream, a.part_sum, a.part_cnt, nblk, HW, mask ? 1 : 0, loss,
                       count);
    return hipGetLastError();
}

hipError_t launch_dpv_soft_ce_backward(const float* logp, const float* d_candi, const float* label, const float* depth_gt,
                                       float variance, float pw, const float* mask, const float* count, int B, int D, int H, int W,
                                       const float* g_loss, const float* g_depth, float* g_logp, hipStream_t stream) {
    const int HW = H * W;
    CeBwdArgs a{};
    a.logp = logp; a.dc = d_candi; a.label = label; a.depth_gt = depth_gt; a.mask = mask; a.count = count;
    a.g_loss = g_loss; a.g_depth = g_depth;
    if (depth_gt) a.gs = make_gauss(variance, pw);
    a.D = D; a.HW = HW; a.g_logp = g_logp;
    const bool vec = (HW % 4 == 0) && D <= 128 && aligned16(logp) && (!label || aligned16(label)) &&
                     (!depth_gt || aligned16(depth_gt)) && (!mask || aligned16(mask)) && (!g_depth || aligned16(g_depth)) &&
                     aligned16(g_logp);
    const dim3 grid(n_blocks(H, W), B);
    if (vec) {
        for_planes_per_lane(D, [&](auto rpl) {
            constexpr int RPL = decltype(rpl)::value;
            if (depth_gt) hipLaunchKernelGGL((soft_ce_bwd_vec4_kernel<true, RPL>), grid, dim3(256), 0, stream, a);
            else hipLaunchKernelGGL((soft_ce_bwd_vec4_kernel<false, RPL>), grid, dim3(256), 0, stream, a);
        });
    } else if (depth_gt) {
        hipLaunchKernelGGL(soft_ce_bwd_scalar_kernel<true>, grid, dim3(256), 0, stream, a);
    } else {
        hipLaunchKernelGGL(soft_ce_bwd_scalar_kernel<false>, grid, dim3(256), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entries live here, beside their kernels: capi.o does not refer to this object, so a
// library linked from a subset of the objects (tests/test_sweep_prefetch.py) still links. ------------------------------------
namespace {

using namespace pdepth::capi;

// what the two cross-entropy entries check alike: the volume, the sizes, the label source
int check_soft_ce(const char* who, const float* logp, const float* d_candi, const float* label, const float* depth_gt, float variance,
                  float pw, int32_t B, int32_t D, int32_t H, int32_t W) {
    if (!logp || !d_candi) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_dims(who, B, D, H, W)) return rc;
    if (int rc = check_launch_limits(who, B, H, W)) return rc;
    if ((label != nullptr) == (depth_gt != nullptr))
        return fail(PDEPTH_E_ARG, "%s: exactly one label source (label or depth_gt) must be given", who);
    if (depth_gt && !(variance > 0.0f)) return fail(PDEPTH_E_ARG, "%s: variance must be positive", who);
    if (depth_gt && !(pw > 0.0f)) return fail(PDEPTH_E_ARG, "%s: pow must be positive", who);
    return PDEPTH_OK;
}
}  // namespace

extern "C" {

size_t pdepth_dpv_soft_ce_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return (B > 0 && H > 0 && W > 0 && (long long)H * W <= (1ll << 30)) ? pdepth::dpv_soft_ce_workspace_bytes(B, H, W) : 0;
}

// soft_cross_entropy_loss(BV_log=True) (losses/loss_blocks.py:186-202) + dpv_to_depthmap (utils/img_utils.py:52-61), the label
// read or formed as gen_soft_label_torch(zero_invalid=True) does (utils/img_utils.py:24-47)
int pdepth_dpv_soft_ce_f32(const float* logp, const float* d_candi, const float* label, const float* depth_gt, float variance,
                           float pow, const float* mask, int32_t B, int32_t D, int32_t H, int32_t W, float* loss, float* count,
                           float* depth, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pdepth_dpv_soft_ce_f32";
    if (int rc = check_soft_ce(who, logp, d_candi, label, depth_gt, variance, pow, B, D, H, W)) return rc;
    if (!loss || !count) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_workspace(who, workspace, workspace_bytes, pdepth::dpv_soft_ce_workspace_bytes(B, H, W))) return rc;
    return launched(pdepth::launch_dpv_soft_ce(logp, d_candi, label, depth_gt, variance, pow, mask, B, D, H, W, loss, count, depth,
                                               workspace, (hipStream_t)stream), who);
}

int pdepth_dpv_soft_ce_backward_f32(const float* logp, const float* d_candi, const float* label, const float* depth_gt, float variance,
                                    float pow, const float* mask, const float* count, int32_t B, int32_t D, int32_t H, int32_t W,
                                    const float* g_loss, const float* g_depth, float* g_logp, void* stream) {
    const char* who = "pdepth_dpv_soft_ce_backward_f32";
    if (int rc = check_soft_ce(who, logp, d_candi, label, depth_gt, variance, pow, B, D, H, W)) return rc;
    if (!count || !g_logp) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!g_loss && !g_depth) return fail(PDEPTH_E_ARG, "%s: no incoming gradient", who);
    if ((const float*)g_logp == logp || (const float*)g_logp == label)
        return fail(PDEPTH_E_ARG, "%s: g_logp may not alias an input", who);
    return launched(pdepth::launch_dpv_soft_ce_backward(logp, d_candi, label, depth_gt, variance, pow, mask, count, B, D, H, W, g_loss,
                                                        g_depth, g_logp, (hipStream_t)stream), who);
}

}  // extern "C"
