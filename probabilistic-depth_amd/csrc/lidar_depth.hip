// Ground truth on the device: a batch of LiDAR scans -> the depth maps and masks of a training / validation step.
//
// Replaces generate_depth (external/utils_lib/python/utils_lib.cpp:86-160, upsample = 0) and what the loader does with its
// result (kittiloader/kitti.py:683-729: util.minpool(large, 4, 1000), utils/img_utils.py:87-95, and the two masks).  Per item:
//   point pass   one thread per point (x, y, z, w), fp32, every product and sum on its own (the library is built with
//                -ffp-contract=off), each chain left to right:
//                    cam_r  = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3] w                 r = 0 .. 3
//                    proj_r = ((I[r][0] cam_0 + I[r][1] cam_1) + I[r][2] cam_2) + I[r][3] cam_3   r = 0 .. 2
//                    u_f = proj_0 / proj_2,  v_f = proj_1 / proj_2                                (IEEE division)
//                kept iff cam_2 >= 0.1 (the reference compares the float with the double 0.1: the same floats pass) and
//                finite.  u = (int)(u_f - 0.5), v = (int)(v_f - 0.5): the reference subtracts the double 0.5, so the
//                difference is exact, and truncates toward zero: a difference in (-1, 1) is column 0, <= -1 and >= W are
//                outside.  The range is tested on the double BEFORE the conversion, so a NaN, an infinity or a position
//                beyond the int range is skipped and never converted.  The depth is cam_2: an unsigned atomicMin of its bit
//                pattern (a positive float orders like its bits) into the z-buffer of the workspace.  The minimum does not depend
//                on the order of the points: two calls give the same bits.
//   map pass     a workgroup owns a 32 x 32 tile of the full-resolution map and stages it, with a halo of f pixels, in LDS.
//                filter: pixel (v, u) is non-zero only for f <= v < H-f-1 and f <= u < W-f-1 (the reference's bounds: the
//                last f+1 rows and columns are zero); there it keeps its z unless another pixel of the (2f+1)^2 window has
//                zn != 0 and zn - z < -filterdiff (strict).  fp32 subtraction is monotone in zn, so the decision is taken on
//                the window's minimum.  The window reads the raw z-buffer: nothing cascades.
//                mask = 1 where the map >= 0.01, the map is multiplied by it; the quarter map is the minimum over 4 x 4 blocks
//                with zeros lifted to pool_default, a block whose minimum equals pool_default becomes 0 (so a depth >= 1000
//                beside an empty pixel disappears, as in the reference); its mask and product likewise.  [H/4] x [W/4]: a
//                ragged remainder is dropped.
// The z-buffer is initialised by a launch of its own (all bits set = empty, above every float's pattern) -- the fill kernel of
// clear.hip, not hipMemsetAsync: with a memset node in front, a captured call replayed on new points did not reproduce the eager
// call (every memset-fronted scatter of the library turned out to behave so, and clear.hip is what they all use
// now).  Nothing is allocated, nothing waits for the host: the call can be captured in a graph.
#include <hip/hip_runtime.h>

#include <cmath>

#include "capi_util.hpp"
#include "kernels.hpp"

namespace pdepth {

namespace {

constexpr unsigned EMPTY = 0xFFFFFFFFu;
constexpr int TILE = 32;        // full-resolution pixels per side of a workgroup's tile (a multiple of 4)
constexpr int MAX_FILTER = 4;

struct LidarArgs {
    const float* points;   // [B,Nmax,dim]
    const int* counts;     // [B]
    const float* M;        // [4,4] or [B,4,4]
    const float* intr;     // [3,4] or [B,3,4]
    int Nmax, dim, M_stride, intr_stride, H, W;
    float filterdiff, pool_default;
    unsigned* zbuf;        // [B,H,W]
    float *dmap, *mask, *dmap_q, *mask_q;
};

__global__ __launch_bounds__(256) void lidar_points_kernel(LidarArgs a) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(a.counts[b], a.Nmax);
    if (i >= n) return;
    const size_t row = (size_t)b * a.Nmax + i;
    float x, y, z, w;
    if (a.dim == 4) {
        const float4 p = reinterpret_cast<const float4*>(a.points)[row];
        x = p.x; y = p.y; z = p.z; w = p.w;
    } else {
        const float* p = a.points + row * 3;
        x = p[0]; y = p[1]; z = p[2]; w = 1.0f;
    }
    const float* M = a.M + (size_t)b * a.M_stride;
    const float* I = a.intr + (size_t)b * a.intr_stride;
    float cam[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) cam[r] = ((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] * w;
    const float cz = cam[2];
    if (!(cz >= 0.1f) || !(cz < INFINITY)) return;
    float pr[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) pr[r] = ((I[4 * r] * cam[0] + I[4 * r + 1] * cam[1]) + I[4 * r + 2] * cam[2]) + I[4 * r + 3] * cam[3];
    const double ud = (double)(pr[0] / pr[2]) - 0.5;
    const double vd = (double)(pr[1] / pr[2]) - 0.5;
    if (!(ud > -1.0 && ud < (double)a.W && vd > -1.0 && vd < (double)a.H)) return;   // (a NaN fails every comparison)
    const int u = (int)ud, v = (int)vd;
    atomicMin(a.zbuf + ((size_t)b * a.H + v) * a.W + u, __float_as_uint(cz));
}

// thread t of the 256: row t / 8 of the tile, columns 4 (t % 8) .. + 3.  A wave holds 8 rows: the four rows of a 4 x 4 block
// sit in lanes that differ in bits 3 and 4
template <int F>
__global__ __launch_bounds__(256) void lidar_maps_kernel(LidarArgs a) {
    constexpr int SIDE = TILE + 2 * F;
    constexpr int PITCH = SIDE + 1;   // odd: the 32 lanes of a half-wave (4 rows x 8 column groups of 4) read 32 banks
    __shared__ unsigned zs[SIDE * PITCH];
    const int H = a.H, W = a.W, b = blockIdx.z;
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    const unsigned* zb = a.zbuf + (size_t)b * H * W;
    for (int i = threadIdx.x; i < SIDE * SIDE; i += 256) {
        const int ly = i / SIDE, lx = i - ly * SIDE;
        const int gy = y0 - F + ly, gx = x0 - F + lx;
        zs[ly * PITCH + lx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? zb[(size_t)gy * W + gx] : EMPTY;
    }
    __syncthreads();
    const int ty = threadIdx.x >> 3, tx = (threadIdx.x & 7) * 4;
    const int gy = y0 + ty, gx = x0 + tx;
    unsigned near[4] = {EMPTY, EMPTY, EMPTY, EMPTY};   // the nearest other pixel of each window
#pragma unroll
    for (int dy = -F; dy <= F; ++dy) {
#pragma unroll
        for (int dx = -F; dx <= F + 3; ++dx) {
            const unsigned zn = zs[(ty + F + dy) * PITCH + tx + F + dx];
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (dx - p >= -F && dx - p <= F && !(dy == 0 && dx == p)) near[p] = min(near[p], zn);
        }
    }
    const bool row_in = gy >= F && gy < H - F - 1;
    float out[4], lifted = INFINITY;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const unsigned zu = zs[(ty + F) * PITCH + tx + F + p];
        float val = 0.0f;
        if (row_in && gx + p >= F && gx + p < W - F - 1 && zu != EMPTY) {
            const float z = __uint_as_float(zu);
            const bool bad = near[p] != EMPTY && (__uint_as_float(near[p]) - z) < -a.filterdiff;
            if (!bad) val = z;
        }
        val = val >= 0.01f ? val : 0.0f;   // the map times its mask
        out[p] = val;
        lifted = fminf(lifted, (val == 0.0f && a.pool_default != 0.0f) ? a.pool_default : val);
    }
    if (gy < H) {
        const size_t o = ((size_t)b * H + gy) * W + gx;
        if ((W & 3) == 0) {   // (then gx < W covers the four, and every row starts 16-byte aligned: the entry checks the bases)
            if (gx < W) {
                *reinterpret_cast<float4*>(a.dmap + o) = make_float4(out[0], out[1], out[2], out[3]);
                *reinterpret_cast<float4*>(a.mask + o) = make_float4(out[0] != 0.0f ? 1.0f : 0.0f, out[1] != 0.0f ? 1.0f : 0.0f,
                                                                      out[2] != 0.0f ? 1.0f : 0.0f, out[3] != 0.0f ? 1.0f : 0.0f);
            }
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (gx + p < W) {
                    a.dmap[o + p] = out[p];
                    a.mask[o + p] = out[p] != 0.0f ? 1.0f : 0.0f;
                }
            }
        }
    }
    // the 4 x 4 block: this lane's four pixels, then the rows in the lanes 8 and 16 away (every lane of the wave is here)
    lifted = fminf(lifted, __shfl_xor(lifted, 8));
    lifted = fminf(lifted, __shfl_xor(lifted, 16));
    const int Hq = H >> 2, Wq = W >> 2, qy = gy >> 2, qx = gx >> 2;
    if ((ty & 3) == 0 && qy < Hq && qx < Wq) {
        float s = lifted == a.pool_default ? 0.0f : lifted;
        s = s >= 0.01f ? s : 0.0f;
        const size_t o = ((size_t)b * Hq + qy) * Wq + qx;
        a.dmap_q[o] = s;
        a.mask_q[o] = s != 0.0f ? 1.0f : 0.0f;
    }
}

}  // namespace

size_t lidar_depth_workspace_bytes(int B, int H, int W) {
    return ((size_t)B * H * W * sizeof(unsigned) + 255) / 256 * 256;
}

hipError_t launch_lidar_depth(const float* points, const int* counts, const float* M, const float* intr, int B, int Nmax,
                              int point_dim, int M_batched, int intr_batched, int H, int W, int filtering, float filterdiff,
                              float pool_default, float* dmap, float* mask, float* dmap_q, float* mask_q, void* workspace,
                              hipStream_t stream) {
    LidarArgs a{};
    a.points = points; a.counts = counts; a.M = M; a.intr = intr;
    a.Nmax = Nmax; a.dim = point_dim; a.M_stride = M_batched ? 16 : 0; a.intr_stride = intr_batched ? 12 : 0; a.H = H; a.W = W;
    a.filterdiff = filterdiff; a.pool_default = pool_default;
    a.zbuf = static_cast<unsigned*>(workspace);
    a.dmap = dmap; a.mask = mask; a.dmap_q = dmap_q; a.mask_q = mask_q;
    hipError_t err = launch_fill32(workspace, EMPTY, lidar_depth_workspace_bytes(B, H, W), stream);   // (clear.hip)
    if (err != hipSuccess) return err;
    if (Nmax > 0) {
        hipLaunchKernelGGL(lidar_points_kernel, dim3((Nmax + 255) / 256, B), dim3(256), 0, stream, a);
        err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    const dim3 grid((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, B);
    switch (filtering) {
        case 0: hipLaunchKernelGGL(lidar_maps_kernel<0>, grid, dim3(256), 0, stream, a); break;
        case 1: hipLaunchKernelGGL(lidar_maps_kernel<1>, grid, dim3(256), 0, stream, a); break;
        case 2: hipLaunchKernelGGL(lidar_maps_kernel<2>, grid, dim3(256), 0, stream, a); break;
        case 3: hipLaunchKernelGGL(lidar_maps_kernel<3>, grid, dim3(256), 0, stream, a); break;
        default: hipLaunchKernelGGL(lidar_maps_kernel<MAX_FILTER>, grid, dim3(256), 0, stream, a); break;
    }
    return hipGetLastError();
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h), beside its kernels like the entries of loss.hip and metrics.hip -------------------------------
using namespace pdepth::capi;

extern "C" {

size_t pdepth_lidar_depth_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return (B > 0 && H > 0 && W > 0 && (long long)H * W <= (1ll << 30)) ? pdepth::lidar_depth_workspace_bytes(B, H, W) : 0;
}

int pdepth_lidar_depth_f32(const float* points, const int32_t* counts, const float* M_velo2cam, const float* intr, int32_t B,
                           int32_t Nmax, int32_t point_dim, int32_t M_batched, int32_t intr_batched, int32_t H, int32_t W,
                           int32_t filtering, float filterdiff, float pool_default, float* dmap, float* mask, float* dmap_quarter,
                           float* mask_quarter, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pdepth_lidar_depth_f32";
    if (!counts || !M_velo2cam || !intr) return fail(PDEPTH_E_ARG, "%s: null pointer (counts, M_velo2cam or intr)", who);
    if (int rc = check_dims(who, B, 1, H, W)) return rc;
    if (Nmax < 0) return fail(PDEPTH_E_ARG, "%s: negative Nmax", who);
    if (Nmax > 0 && !points) return fail(PDEPTH_E_ARG, "%s: null pointer (points)", who);
    if (point_dim != 3 && point_dim != 4) return fail(PDEPTH_E_ARG, "%s: point_dim must be 3 (w = 1) or 4, got %d", who, point_dim);
    if (point_dim == 4 && (reinterpret_cast<uintptr_t>(points) & 15u) != 0)
        return fail(PDEPTH_E_ARG, "%s: points [B,Nmax,4] must be 16-byte aligned", who);
    if (int rc = check_launch_limits(who, B, H, W)) return rc;
    if ((long long)B * H * W > (1ll << 40)) return fail(PDEPTH_E_ARG, "%s: B*H*W must be at most 2^40", who);   // (the clearing launch's grid)
    if (filtering < 0 || filtering > 4)
        return fail(PDEPTH_E_ARG, "%s: filtering must be in 0 .. 4 (the window is staged with its halo), got %d", who, filtering);
    if (!std::isfinite(filterdiff) || !std::isfinite(pool_default))
        return fail(PDEPTH_E_ARG, "%s: filterdiff and pool_default must be finite", who);
    if (!dmap || !mask) return fail(PDEPTH_E_ARG, "%s: null output pointer", who);
    if ((H / 4) * (long long)(W / 4) > 0 && (!dmap_quarter || !mask_quarter))
        return fail(PDEPTH_E_ARG, "%s: null output pointer (quarter resolution)", who);
    if (W % 4 == 0 && ((reinterpret_cast<uintptr_t>(dmap) | reinterpret_cast<uintptr_t>(mask)) & 15u) != 0)
        return fail(PDEPTH_E_ARG, "%s: dmap and mask must be 16-byte aligned when W is a multiple of 4", who);
    if (int rc = check_workspace(who, workspace, workspace_bytes, pdepth::lidar_depth_workspace_bytes(B, H, W))) return rc;
    return launched(pdepth::launch_lidar_depth(points, counts, M_velo2cam, intr, B, Nmax, point_dim, M_batched != 0, intr_batched != 0,
                                               H, W, filtering, filterdiff, pool_default, dmap, mask, dmap_quarter, mask_quarter,
                                               workspace, (hipStream_t)stream), who);
}

}  // extern "C"
