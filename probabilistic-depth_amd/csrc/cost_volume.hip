// The per-level cost volume of the flow network (models/pwclite.py: flow_warp, the correlation, LeakyReLU) in one pass:
//     out = leaky_relu(correlation(x1, flow_warp(x2, flow, pad)), slope)        [B, (2 md + 1)^2, H, W]
// the correlation in the one configuration the network instantiates (kernel 1, both strides 1, pad_size = max_displacement = md
// <= 4): out[b, (tj + md)(2 md + 1) + (ti + md), y, x] = (1 / C) sum_c x1[b,c,y,x] w[b,c,y+tj,x+ti], w the warped x2, zeros
// outside the image.  The warped image and the pre-activation volume never reach global memory.
//
//   forward   block = 16 x 16 output pixels of one item, all (2 md + 1)^2 displacements: 81 accumulators per thread and NO split of
//             the displacement rows over blocks (correlation.hip: correlation_fwd_kernel splits them).  A split stages the x2 tile
//             once per row of displacements; here a staged texel is a warped texel -- a sample chain in double and four gathers
//             per channel instead of one load -- and nine times that is the larger price.  The sample of each of the
//             (16 + 2 md)^2 halo texels (flow_warp_sample.hpp, the chain of flow_warp.hip bit for bit) is formed ONCE, before the
//             channel loop, and kept in registers (at most three texels per thread); per chunk of 8 channels the warped halo
//             tile goes to LDS (18 KiB at md = 4) and the thread's own 8 x1 values to registers (a thread reads x1 at its own
//             pixel only).  Sum over c in ascending order in fp32: a chunk's 8 products by one fma each, the chunks' sums added in
//             turn (a shorter chain of roundings than one fma per channel); times 1 / C, the activation in registers, one store.
//             A halo texel outside the image is the correlation's zero padding: staged as 0 and multiplied (0 x inf = NaN).
//   backward  launch 1, the gather of correlation.hip: correlation_bwd_kernel (block = 16 x 16 pixels x 8 channels, no atomics) over the
//             re-warped x2 halo tile (the same loader) and the x1 halo tile: grad_x1, and g_warp, the gradient of the warped image,
//             from grad_out x (out > 0 ? 1 : slope) -- the factor is read from the saved output (0, -0 and NaN take the slope).
//             launch 2: flow_warp's own backward (flow_warp_launch.hpp) with g_warp as its grad_out: grad_x2 by the float-atomic
//             or the integer-sum scatter, grad_flow per owner.  Without a flow g_warp IS grad_x2 and there is no launch 2.
// Workspace of the backward with a flow: g_warp [B,C,H,W] (256-byte rounded), then, _det only, the workspace of flow_warp's _det.
#include <hip/hip_runtime.h>

#include <cmath>

#include "capi_util.hpp"
#include "flow_warp_launch.hpp"
#include "flow_warp_sample.hpp"

namespace pdepth {

namespace {

constexpr int CT = 16;    // tile edge
constexpr int CCH = 8;    // channels per chunk
constexpr int MDMAX = 4;  // largest max_displacement
constexpr int NTMAX = (CT + 2 * MDMAX) * (CT + 2 * MDMAX);   // texels of the largest halo tile

// One halo texel of the warped x2 tile, fixed for every channel: where it is and, with a flow, its sample.
template <bool WARP>
struct HaloTexel {
    flow::Sample q;   // (WARP only)
    long long at;     // WARP: the channel's element (y0, x0) of the sample, which may lie outside; else the texel itself
    bool live;        // inside the image (outside: the correlation's zero padding)
};

// texel (gy, gx) of item b; idx_ok: the thread has such a texel at all
template <bool WARP>
__device__ __forceinline__ HaloTexel<WARP> halo_texel(const float* __restrict__ flo, int b, int gy, int gx, bool idx_ok,
                                                       const flow::Geometry& g, int pad) {
    HaloTexel<WARP> t;
    const int H = g.H, W = g.W;
    t.live = idx_ok && gx >= 0 && gx < W && gy >= 0 && gy < H;
    t.at = 0;
    if (WARP) {
        const int HW = H * W;
        const int pix = t.live ? gy * W + gx : 0;
        const float* f = flo + (size_t)b * 2 * HW + pix;
        t.q = flow::sample(f[0], f[HW], t.live ? gx : 0, t.live ? gy : 0, g, pad);
        t.at = (long long)t.q.y0 * W + t.q.x0;
    } else if (t.live) {
        t.at = (long long)gy * W + gx;
    }
    return t;
}

// the texel's value in one channel plane
template <bool WARP>
__device__ __forceinline__ float halo_value(const HaloTexel<WARP>& t, const float* __restrict__ plane, int W) {
    if (!t.live) return 0.0f;
    if (WARP) return flow::value(t.q, flow::load(plane, t.at, t.q, W));
    return plane[t.at];
}

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.0f ? v : v * slope; }

template <int MD, bool WARP>
__global__ __launch_bounds__(256) void flow_cost_volume_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                               const float* __restrict__ flo, int C, flow::Geometry g, int pad,
                                                               float slope, float* __restrict__ out) {
    constexpr int ND = 2 * MD + 1, TW = CT + 2 * MD, NT = TW * TW, PER = (NT + 255) / 256;
    __shared__ float t2[CCH * NT];   // [CCH][TW][TW]: the warped x2 tile with its halo
    const int H = g.H, W = g.W, HW = H * W;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * CT, y0 = blockIdx.y * CT, b = blockIdx.z;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < W && y < H;
    const int pix = inside ? y * W + x : 0;

    HaloTexel<WARP> tex[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int idx = threadIdx.x + 256 * k;
        const int ry = idx / TW, rx = idx - ry * TW;
        tex[k] = halo_texel<WARP>(flo, b, y0 - MD + ry, x0 - MD + rx, idx < NT, g, pad);
    }

    float acc[ND * ND];
#pragma unroll
    for (int d = 0; d < ND * ND; ++d) acc[d] = 0.0f;
    const size_t image0 = (size_t)b * C * HW;
    for (int c0 = 0; c0 < C; c0 += CCH) {
        float a[CCH];
#pragma unroll
        for (int cc = 0; cc < CCH; ++cc) a[cc] = (c0 + cc < C && inside) ? x1[image0 + (size_t)(c0 + cc) * HW + pix] : 0.0f;
        __syncthreads();   // the readers of the chunk before
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int idx = threadIdx.x + 256 * k;
            if (idx < NT) {
#pragma unroll
                for (int cc = 0; cc < CCH; ++cc)
                    t2[cc * NT + idx] = c0 + cc < C ? halo_value<WARP>(tex[k], x2 + image0 + (size_t)(c0 + cc) * HW, W) : 0.0f;
            }
        }
        __syncthreads();
        // the chunk's own sum first (one fma per channel, ascending), then one addition into the total: a chain of C / 8 + 8 roundings
        // instead of C (at C = 192 the single chain was four times the error of the torch composition's sum)
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const float* row = t2 + (ty + i) * TW + tx;
            float part[ND];
#pragma unroll
            for (int j = 0; j < ND; ++j) part[j] = a[0] * row[j];
#pragma unroll
            for (int cc = 1; cc < CCH; ++cc)
#pragma unroll
                for (int j = 0; j < ND; ++j) part[j] = __builtin_fmaf(a[cc], row[cc * NT + j], part[j]);
#pragma unroll
            for (int j = 0; j < ND; ++j) acc[i * ND + j] += part[j];
        }
    }
    if (!inside) return;
    const float inv = 1.0f / (float)C;
    float* o = out + (size_t)b * ND * ND * HW + pix;
#pragma unroll
    for (int d = 0; d < ND * ND; ++d) o[(size_t)d * HW] = leaky(acc[d] * inv, slope);
}

// Launch 1 of the backward.  grid (tiles along x, tiles along y, B * chunks of 8 channels); md at run time, LDS for md = 4.
//   g1 (WANT1) = grad_x1[b,c,y,x] = (1 / C) sum_d g[b,d,y,x]           w[b,c,y+dy,x+dx]
//   g2 (WANT2) = g_warp [b,c,y,x] = (1 / C) sum_d g[b,d,y-dy,x-dx]    x1[b,c,y-dy,x-dx]
// g = grad_out (out > 0 ? 1 : slope); per (pixel, channel) the sum runs over d in ascending order, one fma each.  The zeros of the
// padding are multiplied like in correlation_bwd_kernel: +-0 for a finite gradient, NaN for inf or NaN.
template <bool WARP, bool WANT1, bool WANT2>
__global__ __launch_bounds__(256) void flow_cost_volume_bwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                                   const float* __restrict__ flo, const float* __restrict__ outv,
                                                                   const float* __restrict__ go, int C, int md, flow::Geometry g, int pad,
                                                                   float slope, float* __restrict__ g1, float* __restrict__ g2) {
    constexpr int PER = (NTMAX + 255) / 256;
    __shared__ float t1[WANT2 ? CCH * NTMAX : 1];   // [CCH][TW][TW] x1 with halo (for g_warp)
    __shared__ float t2[WANT1 ? CCH * NTMAX : 1];   // [CCH][TW][TW] warped x2 with halo (for grad_x1)
    const int H = g.H, W = g.W, HW = H * W;
    const int TW = CT + 2 * md, NT = TW * TW, nd = 2 * md + 1;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * CT, y0 = blockIdx.y * CT;
    const int nchunk = (C + CCH - 1) / CCH;
    const int c0 = (int)(blockIdx.z % nchunk) * CCH, b = blockIdx.z / nchunk;
    const int x = x0 + tx, y = y0 + ty;
    const size_t image0 = (size_t)b * C * HW;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int idx = threadIdx.x + 256 * k;
        if (idx >= NT) break;
        const int ry = idx / TW, rx = idx - ry * TW;
        const int gy = y0 - md + ry, gx = x0 - md + rx;
        if (WANT1) {
            const HaloTexel<WARP> t = halo_texel<WARP>(flo, b, gy, gx, true, g, pad);
#pragma unroll
            for (int cc = 0; cc < CCH; ++cc)
                t2[cc * NT + idx] = c0 + cc < C ? halo_value<WARP>(t, x2 + image0 + (size_t)(c0 + cc) * HW, W) : 0.0f;
        }
        if (WANT2) {
            const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
#pragma unroll
            for (int cc = 0; cc < CCH; ++cc)
                t1[cc * NT + idx] = (in && c0 + cc < C) ? x1[image0 + (size_t)(c0 + cc) * HW + gy * W + gx] : 0.0f;
        }
    }
    __syncthreads();
    const bool inside = x < W && y < H;
    const float* gb = go + (size_t)b * nd * nd * HW;
    const float* ob = outv + (size_t)b * nd * nd * HW;
    float a1[CCH], a2[CCH];
#pragma unroll
    for (int cc = 0; cc < CCH; ++cc) a1[cc] = a2[cc] = 0.0f;
    for (int i = 0; i < nd; ++i) {
        const int dy = i - md;
        for (int j = 0; j < nd; ++j) {
            const int dx = j - md;
            const size_t plane = (size_t)(i * nd + j) * HW;
            if (WANT1) {
                float gv = 0.0f;
                if (inside) {
                    const float v = gb[plane + y * W + x];
                    gv = ob[plane + y * W + x] > 0.0f ? v : v * slope;
                }
                const float* p = t2 + (ty + md + dy) * TW + (tx + md + dx);
#pragma unroll
                for (int cc = 0; cc < CCH; ++cc) a1[cc] = __builtin_fmaf(gv, p[cc * NT], a1[cc]);
            }
            if (WANT2) {
                const int ym = y - dy, xm = x - dx;   // the x1 position whose pair is (y, x)
                float gv = 0.0f;
                if (inside && ym >= 0 && ym < H && xm >= 0 && xm < W) {
                    const float v = gb[plane + ym * W + xm];
                    gv = ob[plane + ym * W + xm] > 0.0f ? v : v * slope;
                }
                const float* p = t1 + (ty + md - dy) * TW + (tx + md - dx);
#pragma unroll
                for (int cc = 0; cc < CCH; ++cc) a2[cc] = __builtin_fmaf(gv, p[cc * NT], a2[cc]);
            }
        }
    }
    if (!inside) return;
    const float inv = 1.0f / (float)C;
#pragma unroll
    for (int cc = 0; cc < CCH; ++cc) {
        if (c0 + cc >= C) break;
        const size_t o = image0 + (size_t)(c0 + cc) * HW + y * W + x;
        if (WANT1) g1[o] = a1[cc] * inv;
        if (WANT2) g2[o] = a2[cc] * inv;
    }
}

inline flow::Geometry geometry_of(int H, int W, bool warp) { return warp ? flow::geometry(H, W) : flow::Geometry{H, W, 0.0, 0.0}; }
inline dim3 tiles(int H, int W, unsigned z) { return dim3((unsigned)((W + CT - 1) / CT), (unsigned)((H + CT - 1) / CT), z); }

template <int MD>
void launch_forward_md(const float* x1, const float* x2, const float* flo, int B, int C, int H, int W, int pad, float slope, float* out,
                       hipStream_t s) {
    const dim3 grid = tiles(H, W, B);
    if (flo) hipLaunchKernelGGL((flow_cost_volume_kernel<MD, true>), grid, dim3(256), 0, s, x1, x2, flo, C, geometry_of(H, W, true), pad, slope, out);
    else hipLaunchKernelGGL((flow_cost_volume_kernel<MD, false>), grid, dim3(256), 0, s, x1, x2, flo, C, geometry_of(H, W, false), pad, slope, out);
}

void launch_forward(const float* x1, const float* x2, const float* flo, int B, int C, int H, int W, int md, int pad, float slope,
                    float* out, hipStream_t s) {
    switch (md) {
        case 1: return launch_forward_md<1>(x1, x2, flo, B, C, H, W, pad, slope, out, s);
        case 2: return launch_forward_md<2>(x1, x2, flo, B, C, H, W, pad, slope, out, s);
        case 3: return launch_forward_md<3>(x1, x2, flo, B, C, H, W, pad, slope, out, s);
        default: return launch_forward_md<4>(x1, x2, flo, B, C, H, W, pad, slope, out, s);
    }
}

template <bool WARP>
void launch_gather(const float* x1, const float* x2, const float* flo, const float* outv, const float* go, int B, int C, int H, int W,
                   int md, int pad, float slope, float* g1, float* g2, hipStream_t s) {
    const dim3 grid = tiles(H, W, (unsigned)(B * ((C + CCH - 1) / CCH)));
    const flow::Geometry g = geometry_of(H, W, WARP);
    if (g1 && g2) hipLaunchKernelGGL((flow_cost_volume_bwd_kernel<WARP, true, true>), grid, dim3(256), 0, s, x1, x2, flo, outv, go, C, md, g, pad, slope, g1, g2);
    else if (g1) hipLaunchKernelGGL((flow_cost_volume_bwd_kernel<WARP, true, false>), grid, dim3(256), 0, s, x1, x2, flo, outv, go, C, md, g, pad, slope, g1, g2);
    else if (g2) hipLaunchKernelGGL((flow_cost_volume_bwd_kernel<WARP, false, true>), grid, dim3(256), 0, s, x1, x2, flo, outv, go, C, md, g, pad, slope, g1, g2);
}

// what every entry asks of its sizes and scalars alike
int check_cost_volume(const char* who, bool with_flow, int32_t B, int32_t C, int32_t H, int32_t W, int32_t md, float slope, int32_t pad) {
    if (int rc = capi::check_dims(who, B, C, H, W)) return rc;
    if (md < 1 || md > MDMAX) return capi::fail(PDEPTH_E_ARG, "%s: max_displacement must be 1..%d, got %d", who, MDMAX, md);
    if (!(slope >= 0.0f)) return capi::fail(PDEPTH_E_ARG, "%s: negative_slope is NaN or negative", who);
    if (pad != flow::PAD_BORDER && pad != flow::PAD_ZEROS) return capi::fail(PDEPTH_E_ARG, "%s: unknown pad %d", who, pad);
    if (with_flow && (H < 2 || W < 2))
        return capi::fail(PDEPTH_E_ARG, "%s: H and W must be at least 2 with a flow (the grid is normalised by H - 1 and W - 1)", who);
    if (int rc = capi::check_launch_limits(who, B, H, W)) return rc;
    // the grids: tiles of 16 rows along y, items times chunks of 8 channels along z
    if ((H + CT - 1) / CT > 65535 || (long long)B * ((C + CCH - 1) / CCH) > 65535)
        return capi::fail(PDEPTH_E_ARG, "%s: H must be at most 16 * 65535 and B * ceil(C / 8) at most 65535", who);
    return PDEPTH_OK;
}

inline size_t roundup256(size_t n) { return (n + 255) / 256 * 256; }
inline size_t g_warp_bytes(int B, int C, int H, int W) { return roundup256((size_t)B * C * H * W * sizeof(float)); }
inline bool sizes_in_range(int32_t B, int32_t C, int32_t H, int32_t W) {
    return B > 0 && C > 0 && H > 1 && W > 1 && (long long)H * W <= (1ll << 30) && (H + CT - 1) / CT <= 65535 &&
           (long long)B * ((C + CCH - 1) / CCH) <= 65535;
}

// both backward entries: DET selects the scatter of launch 2
template <bool DET>
int backward(const char* who, const char* query, const float* x1, const float* x2, const float* flo, const float* outv, const float* go,
             int32_t B, int32_t C, int32_t H, int32_t W, int32_t md, float slope, int32_t pad, float* g_x1, float* g_x2, float* g_flow,
             void* workspace, size_t given, hipStream_t s) {
    using namespace capi;
    if (!x1 || !x2 || !outv || !go) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!g_x1 && !g_x2 && !g_flow) return fail(PDEPTH_E_ARG, "%s: no gradient requested", who);
    if (!flo && g_flow) return fail(PDEPTH_E_ARG, "%s: grad_flow requested without a flow", who);
    if (int rc = check_cost_volume(who, flo != nullptr, B, C, H, W, md, slope, pad)) return rc;
    if (!flo) {   // no warp: the gradient of the "warped" image is grad_x2
        launch_gather<false>(x1, x2, flo, outv, go, B, C, H, W, md, pad, slope, g_x1, g_x2, s);
        return launched(hipGetLastError(), who);
    }
    const bool second = g_x2 || g_flow;
    float* g_warp = nullptr;
    void* det_ws = nullptr;
    if (second) {
        const size_t head = g_warp_bytes(B, C, H, W);
        const size_t need = head + ((DET && g_x2) ? flow::warp_backward_det_workspace_bytes(B, C, H, W) : 0);
        if (int rc = check_workspace(who, workspace, given, need, query)) return rc;
        g_warp = static_cast<float*>(workspace);
        det_ws = static_cast<char*>(workspace) + head;
    }
    launch_gather<true>(x1, x2, flo, outv, go, B, C, H, W, md, pad, slope, g_x1, g_warp, s);
    if (int rc = launched(hipGetLastError(), who)) return rc;
    if (!second) return PDEPTH_OK;
    if (DET) return launched(flow::launch_warp_backward_det(x2, flo, g_warp, B, C, H, W, pad, g_x2, g_flow, det_ws, s), who);
    return launched(flow::launch_warp_backward(x2, flo, g_warp, B, C, H, W, pad, g_x2, g_flow, s), who);
}

}  // namespace

}  // namespace pdepth

// ---- C ABI (include/pdepth.h) -------------------------------------------------------------------------------------------------------
using namespace pdepth;
using namespace pdepth::capi;

extern "C" {

int pdepth_flow_cost_volume_f32(const float* x1, const float* x2, const float* flow, int32_t B, int32_t C, int32_t H, int32_t W,
                                int32_t max_displacement, float negative_slope, int32_t pad, float* out, void* stream) {
    const char* who = "pdepth_flow_cost_volume_f32";
    if (!x1 || !x2 || !out) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_cost_volume(who, flow != nullptr, B, C, H, W, max_displacement, negative_slope, pad)) return rc;
    launch_forward(x1, x2, flow, B, C, H, W, max_displacement, pad, negative_slope, out, (hipStream_t)stream);
    return launched(hipGetLastError(), who);
}

size_t pdepth_flow_cost_volume_backward_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t with_flow) {
    return (with_flow && sizes_in_range(B, C, H, W)) ? g_warp_bytes(B, C, H, W) : 0;
}

int pdepth_flow_cost_volume_backward_f32(const float* x1, const float* x2, const float* flow, const float* out, const float* grad_out,
                                         int32_t B, int32_t C, int32_t H, int32_t W, int32_t max_displacement, float negative_slope,
                                         int32_t pad, float* grad_x1, float* grad_x2, float* grad_flow, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    return backward<false>("pdepth_flow_cost_volume_backward_f32", "; query pdepth_flow_cost_volume_backward_workspace_bytes()", x1, x2, flow,
                           out, grad_out, B, C, H, W, max_displacement, negative_slope, pad, grad_x1, grad_x2, grad_flow, workspace,
                           workspace_bytes, (hipStream_t)stream);
}

size_t pdepth_flow_cost_volume_backward_det_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t with_flow) {
    return (with_flow && sizes_in_range(B, C, H, W)) ? g_warp_bytes(B, C, H, W) + flow::warp_backward_det_workspace_bytes(B, C, H, W) : 0;
}

int pdepth_flow_cost_volume_backward_det_f32(const float* x1, const float* x2, const float* flow, const float* out, const float* grad_out,
                                             int32_t B, int32_t C, int32_t H, int32_t W, int32_t max_displacement, float negative_slope,
                                             int32_t pad, float* grad_x1, float* grad_x2, float* grad_flow, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    return backward<true>("pdepth_flow_cost_volume_backward_det_f32", "; query pdepth_flow_cost_volume_backward_det_workspace_bytes()", x1, x2,
                          flow, out, grad_out, B, C, H, W, max_displacement, negative_slope, pad, grad_x1, grad_x2, grad_flow, workspace,
                          workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
