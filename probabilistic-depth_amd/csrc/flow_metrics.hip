// Optical-flow evaluation on the device: rescale and resize a predicted flow to the ground truth's size, the end-point error
// per pixel, the masked means and the KITTI outlier rate ("Fl") per item of a batch, without a read-back.
//
// Replaces, per batch, utils/flow_utils.evaluate_flow (utils/flow_utils.py:61-123; the trainers' call:
// trainer/sintel_trainer.py:92-151).  Per item b and ground-truth pixel (y, x) of an H x W map, pred [B,2,h,w]:
//     u' = (u / (float)w) * (float)W,  v' = (v / (float)h) * (float)H                (flow_utils.py:77-80, per tap, that order)
//     (up, vp) = the bilinear sample of (u', v') at sx = (x + 0.5) w / W - 0.5, sy likewise (cv2.resize, INTER_LINEAR:
//                x0 = floor(sx); x0 < 0 -> tap 0 alone; x0 >= w - 1 -> tap w - 1 alone; the two rows first, then the column)
//     epe = sqrtf((up - gu)^2 + (vp - gv)^2)                                         (float, as numpy's float32)
//     bad(m) <=> epe m > 3 && epe m / max(sqrtf(gu^2 + gv^2), 1e-10) > 0.05
// 2-channel truth: S epe over all pixels.  4-channel truth (valid = gt[:,2], noc = gt[:,3]): S epe valid, S valid, S epe noc,
// S noc, S epe (valid - noc), S (valid - noc), #bad(valid); with move_mask also #bad(valid move), #bad(valid (1 - move)),
// S epe valid move, S valid move, S epe valid (1 - move), S valid (1 - move).
//
// The sample position is formed in double from a scale the host divides once (a float position at x = 1000 is 6e-5 of a pixel
// off: more than the four-tap float interpolation loses); its fraction, the weights and the interpolation are float.  Where
// h == H the fraction is 0 and the row tap is the pixel's own: the same-size call reproduces numpy's float32 bits.
//
// One thread per ground-truth pixel in the pixel order of dpv_lanes.hpp (thread_pixel), 256 per workgroup.  Where H W is a
// multiple of 4 and the truth (and the move mask) start on 16 bytes, a workgroup fetches its 256 pixels of every plane of the
// truth with one 16-byte load per thread -- wave p reads plane p, the first wave the move mask as well -- into LDS, and
// every thread takes its pixel's values from there; otherwise every thread loads its own.  Both paths hand the same values to
// the same lanes: the same bits.
//
// Pixel reduction, as metrics.hip: the per-pixel terms are float, their sums double.  Every workgroup writes one record into the
// workspace; a second launch of one workgroup per item adds the records in a fixed order (lanes by xor-shuffles 32 ... 1, then
// (w0 + w1) + (w2 + w3)) and forms the means and rates.  No atomics: two calls give the same bits.
#include <hip/hip_runtime.h>

#include "capi_util.hpp"
#include "dpv_lanes.hpp"
#include "kernels.hpp"

namespace pdepth {

namespace {

// what the truth defines: its two flow channels alone, + valid and noc, + the move mask
enum { FM_UV = 0, FM_MASKS = 1, FM_MOVE = 2 };
// sums of a record per mode (the order of the list above)
template <int MODE> struct RecLen { static constexpr int value = MODE == FM_UV ? 2 : MODE == FM_MASKS ? 7 : 13; };
constexpr int REC_MAX = 13;

// the prediction and where a pixel of the output samples it: s = (i + off) * scale - off (off 0.5: half-pixel centres; 0: align_corners)
struct ResizeArgs {
    const float* flow;   // [B,2,h,w]
    int h, w, H, W;
    double sx, sy, off;
};

struct FlowMetArgs {
    ResizeArgs r;
    const float* gt;     // [B,C,H,W], C = 2 or 4
    const float* move;   // [B,H,W] or nullptr
    int HW, nblk;
    float* flow_up;      // [B,2,H,W] or nullptr
    double* part;        // [B,nblk,record]
};

// the two taps of one axis and the weight of the second (cv2.resize, INTER_LINEAR; align_corners never leaves [0, n - 1])
struct Taps { int i0, i1; float f; };
__device__ __forceinline__ Taps axis_taps(int i, double scale, double off, int n) {
    const double s = ((double)i + off) * scale - off;
    const double fl = floor(s);
    Taps t;
    t.i0 = (int)fl;
    t.f = (float)(s - fl);
    if (t.i0 < 0) { t.i0 = 0; t.f = 0.f; }
    if (t.i0 >= n - 1) { t.i0 = n - 1; t.f = 0.f; }
    t.i1 = t.i0 + 1 < n ? t.i0 + 1 : n - 1;
    return t;
}

// the rescaled, resized flow of item b at pixel (y, x) of the output: the one statement of the sampling, used by both kernels
__device__ __forceinline__ void sample_flow(const ResizeArgs& r, int b, int y, int x, float& up, float& vp) {
    const Taps tx = axis_taps(x, r.sx, r.off, r.w), ty = axis_taps(y, r.sy, r.off, r.h);
    const size_t plane = (size_t)r.h * r.w;
    const float* pu = r.flow + (size_t)b * 2 * plane;
    const size_t r0 = (size_t)ty.i0 * r.w, r1 = (size_t)ty.i1 * r.w;
    const float fw = (float)r.w, fW = (float)r.W, fh = (float)r.h, fH = (float)r.H;
    const float ax = 1.f - tx.f, ay = 1.f - ty.f;
    float out[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* p = pu + c * plane;
        const float den = c == 0 ? fw : fh, num = c == 0 ? fW : fH;
        const float t00 = (p[r0 + tx.i0] / den) * num, t01 = (p[r0 + tx.i1] / den) * num;
        const float t10 = (p[r1 + tx.i0] / den) * num, t11 = (p[r1 + tx.i1] / den) * num;
        const float top = t00 * ax + t01 * tx.f, bot = t10 * ax + t11 * tx.f;
        out[c] = top * ay + bot * ty.f;
    }
    up = out[0];
    vp = out[1];
}

// flow_utils.py:63-68 for one pixel
__device__ __forceinline__ bool bad_pixel(float epe, float m, float gmag) {
    const float em = epe * m;
    return em > 3.0f && em / gmag > 0.05f;
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void flow_metrics_kernel(FlowMetArgs a) {
    constexpr int REC = RecLen<MODE>::value;
    constexpr int C = MODE == FM_UV ? 2 : 4, PLANES = C + (MODE == FM_MOVE ? 1 : 0);
    __shared__ double sw[4][REC];
    __shared__ __attribute__((aligned(16))) float tile[VEC ? PLANES : 1][256];
    const int HW = a.HW, b = blockIdx.y;
    const int lp = thread_pixel() - blockIdx.x * 256, pix = blockIdx.x * 256 + lp;
    const bool live = pix < HW;
    const float* gt = a.gt + (size_t)b * C * HW;
    const float* mv = MODE == FM_MOVE ? a.move + (size_t)b * HW : nullptr;
    float g[PLANES];
    if (VEC) {
        // thread t: plane t / 64 (one plane per wave), quad t % 64 of the workgroup's 256 pixels; H W % 4 == 0: a quad is whole
        const int q4 = (threadIdx.x & 63) * 4, p = threadIdx.x >> 6;
        const bool qlive = blockIdx.x * 256 + q4 < HW;
        if (p < C && qlive) *reinterpret_cast<float4*>(&tile[p][q4]) = load_nt(gt + (size_t)p * HW + blockIdx.x * 256 + q4);
        if (MODE == FM_MOVE && p == 0 && qlive)
            *reinterpret_cast<float4*>(&tile[PLANES - 1][q4]) = load_nt(mv + blockIdx.x * 256 + q4);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < PLANES; ++c) g[c] = live ? tile[c][lp] : 0.f;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = live ? gt[(size_t)c * HW + pix] : 0.f;
        if (MODE == FM_MOVE) g[PLANES - 1] = live ? mv[pix] : 0.f;
    }
    double acc[REC];
#pragma unroll
    for (int j = 0; j < REC; ++j) acc[j] = 0.0;
    if (live) {
        const int y = pix / a.r.W, x = pix - y * a.r.W;
        float up, vp;
        sample_flow(a.r, b, y, x, up, vp);
        if (a.flow_up) {
            float* o = a.flow_up + (size_t)b * 2 * HW + pix;
            o[0] = up;
            o[HW] = vp;
        }
        const float du = up - g[0], dv = vp - g[1];
        const float epe = sqrtf(du * du + dv * dv);
        if (MODE == FM_UV) {
            acc[0] = epe;
            acc[1] = 1.0;
        } else {
            const float valid = g[2], noc = g[3], occ = valid - noc;
            const float gmag = fmaxf(sqrtf(g[0] * g[0] + g[1] * g[1]), 1e-10f);
            acc[0] = epe * valid; acc[1] = valid;
            acc[2] = epe * noc;   acc[3] = noc;
            acc[4] = epe * occ;   acc[5] = occ;
            acc[6] = bad_pixel(epe, valid, gmag) ? 1.0 : 0.0;
            if (MODE == FM_MOVE) {
                const float mvm = valid * g[PLANES - 1], stm = valid * (1.0f - g[PLANES - 1]);
                acc[7] = bad_pixel(epe, mvm, gmag) ? 1.0 : 0.0;
                acc[8] = bad_pixel(epe, stm, gmag) ? 1.0 : 0.0;
                acc[9] = epe * valid * g[PLANES - 1];           acc[10] = mvm;
                acc[11] = epe * valid * (1.0f - g[PLANES - 1]); acc[12] = stm;
            }
        }
    }
    // the record of the workgroup -> its slot of the workspace (the order of metrics.hip: block_record)
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

// one workgroup per item: the records in a fixed order -> errors[b, 0..7], counts[b, 0..4]
template <int MODE>
__global__ __launch_bounds__(256) void flow_metrics_final_kernel(const double* __restrict__ part, int nblk, float* __restrict__ errors,
                                                                 float* __restrict__ counts) {
    constexpr int REC = RecLen<MODE>::value;
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
    for (int j = 0; j < REC; ++j) {
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
        float* e = errors + (size_t)b * 8;
        float* n = counts + (size_t)b * 5;
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = nan;
#pragma unroll
        for (int j = 0; j < 5; ++j) n[j] = nan;
        // a sum over no pixel divides 0 by 0: NaN, where numpy divides by zero
        e[0] = (float)(S[0] / S[1]);
        n[0] = (float)S[1];
        if (MODE != FM_UV) {
            e[1] = (float)(S[2] / S[3]);
            e[2] = (float)(S[4] / (S[5] > 1.0 ? S[5] : 1.0));   // (flow_utils.py:95-96)
            e[3] = (float)(S[6] / S[1] * 100.0);
            n[1] = (float)S[3];
            n[2] = (float)S[5];
        }
        if (MODE == FM_MOVE) {
            e[4] = (float)(S[9] / S[10]);
            e[5] = (float)(S[11] / S[12]);
            e[6] = (float)(S[7] / S[10] * 100.0);
            e[7] = (float)(S[8] / S[12] * 100.0);
            n[3] = (float)S[10];
            n[4] = (float)S[12];
        }
    }
}

// rescale + resize alone: out [B,2,H,W]
__global__ __launch_bounds__(256) void flow_resize_kernel(ResizeArgs r, int HW, float* __restrict__ out) {
    const int pix = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (pix >= HW) return;
    const int y = pix / r.W, x = pix - y * r.W;
    float up, vp;
    sample_flow(r, b, y, x, up, vp);
    float* o = out + (size_t)b * 2 * HW + pix;
    o[0] = up;
    o[HW] = vp;
}

ResizeArgs resize_args(const float* flow, int h, int w, int H, int W, bool align_corners) {
    ResizeArgs r{};
    r.flow = flow; r.h = h; r.w = w; r.H = H; r.W = W;
    if (align_corners) {
        r.off = 0.0;
        r.sx = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
        r.sy = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0;
    } else {
        r.off = 0.5;
        r.sx = (double)w / (double)W;
        r.sy = (double)h / (double)H;
    }
    return r;
}

template <int MODE>
hipError_t launch_mode(const FlowMetArgs& a, bool vec, int B, float* errors, float* counts, hipStream_t stream) {
    const dim3 grid(a.nblk, B);
    if (vec) hipLaunchKernelGGL((flow_metrics_kernel<MODE, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((flow_metrics_kernel<MODE, false>), grid, dim3(256), 0, stream, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(flow_metrics_final_kernel<MODE>, dim3(B), dim3(256), 0, stream, a.part, a.nblk, errors, counts);
    return hipGetLastError();
}

}  // namespace

size_t flow_metrics_workspace_bytes(int B, int H, int W) {
    const size_t n = (size_t)B * n_blocks(H, W);
    return (n * REC_MAX * sizeof(double) + 255) / 256 * 256;
}

hipError_t launch_flow_metrics(const float* gt, int gt_channels, const float* pred, int h, int w, const float* move_mask, int B, int H,
                               int W, float* errors, float* counts, float* flow_up, void* workspace, hipStream_t stream) {
    FlowMetArgs a{};
    a.r = resize_args(pred, h, w, H, W, false);
    a.gt = gt; a.move = move_mask; a.HW = H * W; a.nblk = n_blocks(H, W); a.flow_up = flow_up;
    a.part = static_cast<double*>(workspace);
    const bool vec = (a.HW % 4 == 0) && aligned16(gt) && (!move_mask || aligned16(move_mask));   // (as launch_depth_metrics decides)
    if (gt_channels == 2) return launch_mode<FM_UV>(a, vec, B, errors, counts, stream);
    if (!move_mask) return launch_mode<FM_MASKS>(a, vec, B, errors, counts, stream);
    return launch_mode<FM_MOVE>(a, vec, B, errors, counts, stream);
}

hipError_t launch_flow_resize(const float* flow, int B, int h, int w, int H, int W, bool align_corners, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(flow_resize_kernel, dim3(n_blocks(H, W), B), dim3(256), 0, stream, resize_args(flow, h, w, H, W, align_corners),
                       H * W, out);
    return hipGetLastError();
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h).  The entries live here, beside their kernels, as those of metrics.hip do. -------------------------
using namespace pdepth::capi;

extern "C" {

size_t pdepth_flow_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return (B > 0 && H > 0 && W > 0 && (long long)H * W <= (1ll << 30)) ? pdepth::flow_metrics_workspace_bytes(B, H, W) : 0;
}

int pdepth_flow_metrics_f32(const float* gt, int32_t gt_channels, const float* pred, int32_t h, int32_t w, const float* move_mask,
                            int32_t B, int32_t H, int32_t W, float* errors, float* counts, float* flow_up, void* workspace,
                            size_t workspace_bytes, void* stream) {
    const char* who = "pdepth_flow_metrics_f32";
    if (!gt || !pred) return fail(PDEPTH_E_ARG, "%s: null pointer (gt or pred)", who);
    if (gt_channels != 2 && gt_channels != 4)
        return fail(PDEPTH_E_ARG, "%s: gt_channels=%d: the truth has 2 channels (u, v) or 4 (u, v, valid, noc)", who, gt_channels);
    if (move_mask && gt_channels != 4) return fail(PDEPTH_E_ARG, "%s: a move mask needs a truth of 4 channels (it multiplies valid)", who);
    if (int rc = check_dims(who, B, 1, H, W)) return rc;
    if (int rc = check_dims(who, B, 1, h, w)) return rc;
    if (int rc = check_launch_limits(who, B, H, W)) return rc;
    if (int rc = check_launch_limits(who, B, h, w)) return rc;
    if (!errors || !counts) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (int rc = check_workspace(who, workspace, workspace_bytes, pdepth::flow_metrics_workspace_bytes(B, H, W))) return rc;
    return launched(pdepth::launch_flow_metrics(gt, gt_channels, pred, h, w, move_mask, B, H, W, errors, counts, flow_up, workspace,
                                                (hipStream_t)stream), who);
}

int pdepth_flow_resize_f32(const float* flow, int32_t B, int32_t h, int32_t w, int32_t H, int32_t W, int32_t align_corners, float* out,
                           void* stream) {
    const char* who = "pdepth_flow_resize_f32";
    if (!flow) return fail(PDEPTH_E_ARG, "%s: null pointer (flow)", who);
    if (int rc = check_dims(who, B, 1, H, W)) return rc;
    if (int rc = check_dims(who, B, 1, h, w)) return rc;
    if (int rc = check_launch_limits(who, B, H, W)) return rc;
    if (int rc = check_launch_limits(who, B, h, w)) return rc;
    if (align_corners != 0 && align_corners != 1) return fail(PDEPTH_E_ARG, "%s: align_corners=%d must be 0 or 1", who, align_corners);
    if (!out) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if (out == flow) return fail(PDEPTH_E_ARG, "%s: the output may not alias the input", who);
    return launched(pdepth::launch_flow_resize(flow, B, h, w, H, W, align_corners != 0, out, (hipStream_t)stream), who);
}

}  // extern "C"
