// flow_warp (utils/warp_utils.py:82-89) and the forward-backward check (:92-99) of the unsupervised flow loss
// (losses/flow_loss.py): x [B,C,H,W] sampled bilinearly at base grid + flow [B,2,H,W], border or zeros padding.
//
// The per-sample chain -- position, clamp, taps, weights, value and its derivatives -- is flow_warp_sample.hpp, run by every
// kernel here: the backward scatters through the forward's taps bit for bit.
//   forward     one thread per pixel: the sample once, then its channels, four gathers each.  Lanes run along W: coalesced stores,
//               and for a smooth flow nearly coalesced gathers.  grid (blocks of 256 pixels, channel chunks, B): a thread takes
//               channels chunk, chunk + nchunk, ... -- at the flow network's coarse levels (C = 192 at 4 x 8) pixels alone leave
//               the chip empty.
//   grad_flow   per owner: one thread sums d value / d (ix, iy) g over all channels of its pixel, in channel order.  No atomics:
//               the same bits from call to call.
//   grad_x      a scatter of g w_t to the in-bounds taps (flow::scatter), the forward's grid, into one of the three sinks of
//               fixed_accum.hpp: FloatAtomics (grad_x zeroed on the stream first; the last bits depend on the order of arrival), or
//               MaxOfAbs and IntegerSum, the two passes of the deterministic form (max_exponent_pass, max_exponent_scatter):
//               S_b from the exact maximum of |q| of the item and N = 4 H W.
//   fb check    one thread per pixel: the two channels of flow21 at base + flow12, zeros padding, and the comparison.
// Workspace of the deterministic form: a 256-byte-rounded header of 4 bytes per item, then one int64 per element of grad_x.
#include <hip/hip_runtime.h>

#include <cmath>

#include "capi_util.hpp"
#include "fixed_accum.hpp"
#include "flow_warp_launch.hpp"
#include "flow_warp_sample.hpp"

namespace pdepth {

namespace {

using namespace fixed;

// the most contributions one element of grad_x can receive (the kernels' and the convert pass's exponents both come from it)
__host__ __device__ inline long long max_contributions(int H, int W) { return 4ll * H * W; }

size_t workspace_bytes(int B, size_t per_item) { return det_workspace_bytes(B, MaxExponent::WORDS, per_item); }

// channel chunks (grid y): at least ~1024 workgroups where the channels allow it, at most 64 chunks
inline int channel_chunks(int B, int C, int H, int W) {
    const long long blocks = (((long long)H * W + 255) / 256) * B;
    long long n = 1024 / blocks;
    n = n < 1 ? 1 : n > 64 ? 64 : n;
    return (int)(n > C ? C : n);
}
inline dim3 grid_of(int B, int H, int W, int nchunk) { return dim3((unsigned)(((size_t)H * W + 255) / 256), nchunk, B); }

// the sample of the thread's pixel (pix < H W) of item b
__device__ __forceinline__ flow::Sample pixel_sample(const float* __restrict__ flo, int b, int pix, const flow::Geometry& g, int pad) {
    const int HW = g.H * g.W;
    const int y = pix / g.W, x = pix - y * g.W;
    const float* f = flo + (size_t)b * 2 * HW + pix;
    return flow::sample(f[0], f[HW], x, y, g, pad);
}

__global__ __launch_bounds__(256) void flow_warp_kernel(const float* __restrict__ x, const float* __restrict__ flo, int C,
                                                        flow::Geometry g, int pad, float* __restrict__ out) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int H = g.H, W = g.W, HW = H * W;
    if (pix >= HW) return;
    const int b = blockIdx.z;
    const flow::Sample q = pixel_sample(flo, b, pix, g, pad);
    const long long tap = (long long)q.y0 * W + q.x0;
    const size_t image0 = (size_t)b * C * HW;
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
        const size_t plane = image0 + (size_t)c * HW;
        out[plane + pix] = flow::value(q, flow::load(x + plane, tap, q, W));
    }
}

// grad_x: every lane of every wave reaches the sink (max_exponent_pass shuffles across the wave): a lane past the map shadows the
// last pixel and adds nothing.  Only in-bounds taps are formed, so every index handed to the sink lies inside the sample's own
// (b, c) plane.
template <class Sink>
__device__ __forceinline__ void flow_warp_bwd_body(const float* __restrict__ flo, const float* __restrict__ gout, int C,
                                                   const flow::Geometry& g, int pad, Sink& sink) {
    const int H = g.H, W = g.W, HW = H * W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const bool live = pix < HW;
    const int pc = live ? pix : HW - 1;
    const int b = blockIdx.z;
    const flow::Sample q = pixel_sample(flo, b, pc, g, pad);
    if (!live || !q.any()) return;
    const long long tap = (long long)q.y0 * W + q.x0;
    const long long image0 = (long long)b * C * HW;
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
        const long long plane = image0 + (long long)c * HW;
        flow::scatter(q, plane + tap, W, gout[plane + pc], sink);
    }
}

__global__ __launch_bounds__(256) void flow_warp_bwd_kernel(const float* __restrict__ flo, const float* __restrict__ gout, int C,
                                                            flow::Geometry g, int pad, float* __restrict__ gx) {
    FloatAtomics sink{gx};
    flow_warp_bwd_body(flo, gout, C, g, pad, sink);
}

// PASS 0: maximum of |q| per item; PASS 1: the integer scatter
template <int PASS>
__global__ __launch_bounds__(256) void flow_warp_bwd_det_kernel(const float* __restrict__ flo, const float* __restrict__ gout, int C,
                                                                flow::Geometry g, int pad, uint32_t* __restrict__ hdr,
                                                                unsigned long long* __restrict__ acc) {
    max_exponent_pass<PASS>(hdr + blockIdx.z, acc, max_contributions(g.H, g.W),
                            [&](auto& sink) { flow_warp_bwd_body(flo, gout, C, g, pad, sink); });
}

// grad_flow [B,2,H,W]: grid (blocks of 256 pixels, 1, B)
__global__ __launch_bounds__(256) void flow_warp_grad_flow_kernel(const float* __restrict__ x, const float* __restrict__ flo,
                                                                  const float* __restrict__ gout, int C, flow::Geometry g, int pad,
                                                                  float* __restrict__ gflow) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int H = g.H, W = g.W, HW = H * W;
    if (pix >= HW) return;
    const int b = blockIdx.z;
    const flow::Sample q = pixel_sample(flo, b, pix, g, pad);
    float gix = 0.0f, giy = 0.0f;
    if (q.any()) {
        const long long tap = (long long)q.y0 * W + q.x0;
        const size_t image0 = (size_t)b * C * HW;
        for (int c = 0; c < C; ++c) {
            const size_t plane = image0 + (size_t)c * HW;
            const flow::Texels v = flow::load(x + plane, tap, q, W);
            const float gv = gout[plane + pix];
            gix += flow::d_ix(q, v) * gv;
            giy += flow::d_iy(q, v) * gv;
        }
    }
    float* gf = gflow + (size_t)b * 2 * HW + pix;
    gf[0] = ((gix * ((float)W / 2.0f)) * q.mx) * 2.0f / (float)(W - 1);
    gf[HW] = ((giy * ((float)H / 2.0f)) * q.my) * 2.0f / (float)(H - 1);
}

// occ = |f12 + w|^2 > scale (|f12|^2 + |w|^2) + bias, w = flow21 sampled at base + flow12 with zeros padding
__global__ __launch_bounds__(256) void flow_fb_check_kernel(const float* __restrict__ flow12, const float* __restrict__ flow21,
                                                            flow::Geometry g, float scale, float bias, float* __restrict__ occ) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int H = g.H, W = g.W, HW = H * W;
    if (pix >= HW) return;
    const int b = blockIdx.z;
    const size_t item0 = (size_t)b * 2 * HW;
    const float fx = flow12[item0 + pix], fy = flow12[item0 + HW + pix];
    const int y = pix / W, x = pix - y * W;
    const flow::Sample q = flow::sample(fx, fy, x, y, g, flow::PAD_ZEROS);
    const long long tap = (long long)q.y0 * W + q.x0;
    const float wx = flow::value(q, flow::load(flow21 + item0, tap, q, W));
    const float wy = flow::value(q, flow::load(flow21 + item0 + HW, tap, q, W));
    const float sx = fx + wx, sy = fy + wy;
    const float mag = (fx * fx + fy * fy) + (wx * wx + wy * wy);
    occ[(size_t)b * HW + pix] = (sx * sx + sy * sy) > scale * mag + bias ? 1.0f : 0.0f;
}

void launch_grad_flow(const float* x, const float* flo, const float* gout, int B, int C, int H, int W, int pad, float* gflow, hipStream_t s) {
    hipLaunchKernelGGL(flow_warp_grad_flow_kernel, grid_of(B, H, W, 1), dim3(256), 0, s, x, flo, gout, C, flow::geometry(H, W), pad, gflow);
}

}  // namespace

// ---- the host side of the backward (flow_warp_launch.hpp): the entries below and those of cost_volume.hip ---------------------------
namespace flow {

int check_flow_warp(const char* who, int32_t B, int32_t C, int32_t H, int32_t W, int32_t pad) {
    if (int rc = capi::check_dims(who, B, C, H, W)) return rc;
    if (H < 2 || W < 2) return capi::fail(PDEPTH_E_ARG, "%s: H and W must be at least 2 (the grid is normalised by H - 1 and W - 1)", who);
    if (pad != flow::PAD_BORDER && pad != flow::PAD_ZEROS) return capi::fail(PDEPTH_E_ARG, "%s: unknown pad %d", who, pad);
    return capi::check_launch_limits(who, B, H, W);
}

hipError_t launch_warp_backward(const float* x, const float* flo, const float* gout, int B, int C, int H, int W, int pad, float* gx,
                                float* gflow, hipStream_t s) {
    if (gflow) launch_grad_flow(x, flo, gout, B, C, H, W, pad, gflow, s);
    if (gx) {
        if (hipError_t e = launch_zero(gx, (size_t)B * C * H * W * sizeof(float), s)) return e;
        hipLaunchKernelGGL(flow_warp_bwd_kernel, grid_of(B, H, W, channel_chunks(B, C, H, W)), dim3(256), 0, s, flo, gout, C,
                           flow::geometry(H, W), pad, gx);
    }
    return hipGetLastError();
}

size_t warp_backward_det_workspace_bytes(int B, int C, int H, int W) { return workspace_bytes(B, (size_t)C * H * W); }

hipError_t launch_warp_backward_det(const float* x, const float* flo, const float* gout, int B, int C, int H, int W, int pad, float* gx,
                                    float* gflow, void* workspace, hipStream_t s) {
    if (gflow) {   // written per owner: the kernel of the atomic entry, nothing scattered
        launch_grad_flow(x, flo, gout, B, C, H, W, pad, gflow, s);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (!gx) return hipSuccess;
    const dim3 grid = grid_of(B, H, W, channel_chunks(B, C, H, W));
    auto launch = [&](auto pass, uint32_t* hdr, unsigned long long* acc) {
        hipLaunchKernelGGL(flow_warp_bwd_det_kernel<decltype(pass)::value>, grid, dim3(256), 0, s, flo, gout, C, flow::geometry(H, W), pad,
                           hdr, acc);
    };
    return max_exponent_scatter(workspace, B, (size_t)C * H * W, max_contributions(H, W), gx, s, launch);
}

}  // namespace flow

}  // namespace pdepth

// ---- C ABI (include/pdepth.h), beside the kernels like the entries of occlusion.hip -------------------------------------------------
using namespace pdepth;
using namespace pdepth::capi;
using pdepth::flow::check_flow_warp;

extern "C" {

int pdepth_flow_warp_f32(const float* x, const float* flow, int32_t B, int32_t C, int32_t H, int32_t W, int32_t pad, float* out,
                         void* stream) {
    const char* who = "pdepth_flow_warp_f32";
    if (!x || !flow || !out) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_flow_warp(who, B, C, H, W, pad)) return rc;
    hipLaunchKernelGGL(flow_warp_kernel, grid_of(B, H, W, channel_chunks(B, C, H, W)), dim3(256), 0, (hipStream_t)stream, x, flow, C,
                       flow::geometry(H, W), pad, out);
    return launched(hipGetLastError(), who);
}

int pdepth_flow_warp_backward_f32(const float* x, const float* flow, const float* grad_out, int32_t B, int32_t C, int32_t H, int32_t W,
                                  int32_t pad, float* grad_x, float* grad_flow, void* stream) {
    const char* who = "pdepth_flow_warp_backward_f32";
    if (!x || !flow || !grad_out) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!grad_x && !grad_flow) return fail(PDEPTH_E_ARG, "%s: no gradient requested", who);
    if (int rc = check_flow_warp(who, B, C, H, W, pad)) return rc;
    return launched(flow::launch_warp_backward(x, flow, grad_out, B, C, H, W, pad, grad_x, grad_flow, (hipStream_t)stream), who);
}

size_t pdepth_flow_warp_backward_det_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    return (B > 0 && B <= 65535 && C > 0 && H > 1 && W > 1 && (long long)H * W <= (1ll << 30)) ? workspace_bytes(B, (size_t)C * H * W) : 0;
}

int pdepth_flow_warp_backward_det_f32(const float* x, const float* flow, const float* grad_out, int32_t B, int32_t C, int32_t H, int32_t W,
                                      int32_t pad, float* grad_x, float* grad_flow, void* workspace, size_t workspace_bytes_given,
                                      void* stream) {
    const char* who = "pdepth_flow_warp_backward_det_f32";
    if (!x || !flow || !grad_out) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!grad_x && !grad_flow) return fail(PDEPTH_E_ARG, "%s: no gradient requested", who);
    if (int rc = check_flow_warp(who, B, C, H, W, pad)) return rc;
    if (grad_x) {
        if (int rc = check_workspace(who, workspace, workspace_bytes_given, workspace_bytes(B, (size_t)C * H * W),
                                     "; query pdepth_flow_warp_backward_det_workspace_bytes()"))
            return rc;
    }
    return launched(flow::launch_warp_backward_det(x, flow, grad_out, B, C, H, W, pad, grad_x, grad_flow, workspace, (hipStream_t)stream), who);
}

int pdepth_flow_fb_check_f32(const float* flow12, const float* flow21, int32_t B, int32_t H, int32_t W, float scale, float bias,
                             float* occ, void* stream) {
    const char* who = "pdepth_flow_fb_check_f32";
    if (!flow12 || !flow21 || !occ) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_flow_warp(who, B, 2, H, W, flow::PAD_ZEROS)) return rc;
    if (std::isnan(scale) || std::isnan(bias)) return fail(PDEPTH_E_ARG, "%s: scale or bias is NaN", who);
    hipLaunchKernelGGL(flow_fb_check_kernel, grid_of(B, H, W, 1), dim3(256), 0, (hipStream_t)stream, flow12, flow21, flow::geometry(H, W), scale,
                       bias, occ);
    return launched(hipGetLastError(), who);
}

}  // extern "C"
