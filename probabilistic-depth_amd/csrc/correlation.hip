// The FlowNet / PWC correlation op in the configuration the flow network instantiates (kernel 1, stride1 1, pad = max_displacement:
// pwclite.py:123-125; models/pwclite.py runs it on every level): the LDS-tiled forward, the matrix-pipe forward and the gather
// backward, their launchers, the choice of kernel for a call, and the C entries of the op (pdepth_correlation_output_size,
// pdepth_correlation_{forward,backward}_{f32,f16}).  Every other configuration, fp16 I/O, and a tile that does not fit the LDS
// run the general kernels of correlation_general.hip.
//
// Replaces the reference's only native operator (models/correlation_package/correlation_cuda_kernel.cu:41-114 forward, :116-300
// backward; semantics pinned by models/correlation_native.py:13-23):
//   out[b, (dy+r)*(2r+1) + (dx+r), y, x] = mean_c x1[b,c,y,x] * x2[b,c,y+dy*s2,x+dx*s2] (zero padded).
#include <hip/hip_runtime.h>

#include "capi_util.hpp"

namespace pdepth {

// ---------------------------------------------------------------------------------------------------
// correlation forward: block = 16x16 output pixels x ONE row of displacements (dy); the x2 tile of that row (halo in
// x only) and the x1 tile of a channel chunk are staged in LDS; every thread keeps the 2r+1 <= 9 sums of its pixel
// and row in registers.  Splitting the displacement rows over blocks gives (2r+1) x more workgroups (a 64x128 map has
// only 32 tiles) and 9 instead of 81 live accumulators; the price is that the x2 rows are staged once per row of
// displacements (from L2).  Sum over c in ascending order, one fma each, scaled by 1/C at the end.
// ---------------------------------------------------------------------------------------------------
constexpr int CT = 16;       // tile edge
constexpr int CCH = 8;       // channels per chunk
constexpr int RMAX = 4;      // max displacement radius (in units of stride2)

// Dynamic LDS of the two tiled kernels, stated once: the launchers and the dispatch below (through the two predicates) read it
// here.  Above 64 KiB a launch opts in with hipFuncSetAttribute; above CORR_LDS_CAP (the CU's 160 KiB) there is no launch: the
// dispatch asks the predicates BEFORE it launches anything and gives such a call to the general kernels.
//   forward  (scalar kernel): (8 * 16 * (16 + 2 md) + 8 * 256) * 4 bytes -- over 64 KiB from md = 49, over the cap from md = 145
//   backward                : 2 * 8 * (16 + 2 md)^2 * 4 bytes            -- over 64 KiB from md = 9,  over the cap from md = 18
constexpr size_t CORR_LDS_CAP = 160 * 1024;
static size_t correlation_forward_lds(int radius, int stride2) {
    const size_t TW = (size_t)CT + 2 * (size_t)radius * (size_t)stride2;
    return ((size_t)CCH * CT * TW + (size_t)CCH * 256) * sizeof(float);
}
static size_t correlation_backward_lds(int radius, int stride2) {
    const size_t TWH = (size_t)CT + 2 * (size_t)radius * (size_t)stride2;
    return (size_t)2 * CCH * TWH * TWH * sizeof(float);
}
static bool correlation_forward_fits(int radius, int stride2) { return correlation_forward_lds(radius, stride2) <= CORR_LDS_CAP; }
static bool correlation_backward_fits(int radius, int stride2) { return correlation_backward_lds(radius, stride2) <= CORR_LDS_CAP; }

template <int R>
__global__ __launch_bounds__(256) void correlation_fwd_kernel(const float* __restrict__ x1,
                                                              const float* __restrict__ x2, int C, int H, int W,
                                                              int s2, float* __restrict__ out) {
    extern __shared__ float smem[];
    constexpr int ND = 2 * R + 1;
    const int halo = R * s2;
    const int TW = CT + 2 * halo;            // row length of the x2 tile
    float* t2 = smem;                        // [CCH][CT][TW]
    float* t1 = smem + CCH * CT * TW;        // [CCH][CT*CT]
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * CT, y0 = blockIdx.y * CT;
    const int i = blockIdx.z % ND, b = blockIdx.z / ND;
    const int dy = (i - R) * s2;
    const int x = x0 + tx, y = y0 + ty;
    const int HW = H * W;
    float acc[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) acc[j] = 0.0f;
    for (int c0 = 0; c0 < C; c0 += CCH) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < CCH * CT * TW; idx += 256) {
            const int cc = idx / (CT * TW), rem = idx - cc * CT * TW;
            const int ry = rem / TW, rx = rem - ry * TW;
            const int gx = x0 - halo + rx, gy = y0 + dy + ry, c = c0 + cc;
            t2[idx] = (c < C && gx >= 0 && gx < W && gy >= 0 && gy < H) ? x2[((size_t)b * C + c) * HW + gy * W + gx] : 0.0f;
        }
#pragma unroll
        for (int cc = 0; cc < CCH; ++cc) {
            const int c = c0 + cc;
            t1[cc * 256 + threadIdx.x] = (c < C && x < W && y < H) ? x1[((size_t)b * C + c) * HW + y * W + x] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < CCH; ++cc) {
            const float a = t1[cc * 256 + threadIdx.x];
            const float* row = t2 + (cc * CT + ty) * TW + tx;
#pragma unroll
            for (int j = 0; j < ND; ++j) acc[j] = __builtin_fmaf(a, row[j * s2], acc[j]);
        }
    }
    if (x < W && y < H) {
        const float inv = 1.0f / (float)C;
#pragma unroll
        for (int j = 0; j < ND; ++j) out[((size_t)b * ND * ND + i * ND + j) * HW + y * W + x] = acc[j] * inv;
    }
}

// ---------------------------------------------------------------------------------------------------
// correlation forward on the matrix pipe (C <= 256, max_displacement <= 16): the sum over the channels is a contraction,
// and for 16 neighbouring pixels of a row the texels of one displacement row they multiply with are 16 + 2 * max_displacement
// consecutive texels -- a banded 16 x (16 + 2 md) x C matrix product.  v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32
// accumulation) computes it in ceil((16 + 2 md) / 16) blocks of 16 texels; of the 16 x 16 results of a block the (pixel,
// texel) pairs on the band's 2 r + 1 diagonals are outputs, the rest is matrix-pipe time nothing else wants.
//   wave  = 16 pixels of one image row, all displacement rows in turn (4 waves per workgroup: 4 pixel groups of the row);
//   B operand = x1[4 k + kq][y][x0 + n], held in registers for the whole wave (C / 4 of them);
//   A operand = x2[4 k + kq][y + dy][t0 + m] by buffer_load_dword (16 lanes = 64 contiguous bytes; outside the image:
//               out-of-range offset = 0 = the zero padding);
//   results pass through 9 x 16 floats of LDS per wave so that every displacement plane gets 64-byte row segments.
// ---------------------------------------------------------------------------------------------------
typedef float corr_v4f __attribute__((ext_vector_type(4)));
template <int KMAX>   // channel groups of 4 held in registers: C <= 4 * KMAX
__global__ __launch_bounds__(256) void correlation_fwd_mfma_kernel(const float* __restrict__ x1, const float* __restrict__ x2, int C, int H,
                                                                   int W, int r, int s2, float* __restrict__ out) {
    __shared__ float tr[4][9 * 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kq = lane >> 4;
    const int HW = H * W, md = r * s2, ND = 2 * r + 1, nk = (C + 3) / 4, nblk = (16 + 2 * md + 15) / 16;
    const int xblocks = (W + 63) / 64;
    const int b = blockIdx.x / (H * xblocks), rem = blockIdx.x - b * (H * xblocks), y = rem / xblocks;
    const int x0 = (rem - y * xblocks) * 64 + wave * 16;
    if (x0 >= W) return;   // (wave-uniform; no barrier in this kernel)
    const int OOBO = 0x7fffffff;
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc((void*)(x1 + (size_t)b * C * HW), 0, C * HW * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc((void*)(x2 + (size_t)b * C * HW), 0, C * HW * 4, 0x00020000);
    float Rb[KMAX];
    {
        const bool okp = x0 + n < W;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int c = 4 * k + kq;
            Rb[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r1, (k < nk && c < C && okp) ? (c * HW + y * W + x0 + n) * 4 : OOBO, 0, 0));
        }
    }
    const float inv = 1.0f / (float)C;
    float* const t = tr[wave];
    for (int di = 0; di < ND; ++di) {
        const int row2 = y + (di - r) * s2;
        const bool rowok = (unsigned)row2 < (unsigned)H;
        for (int blk = 0; blk < nblk; ++blk) {
            // four interleaved chains (pairwise at the end): a quarter of the additions per chain keeps the rounding of a
            // 256-channel sum inside the reference's own 1e-7 self-check bound, and four matrix instructions are independent
            corr_v4f accs[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) accs[q] = corr_v4f{0.f, 0.f, 0.f, 0.f};
            const int tx = x0 - md + 16 * blk + n;
            const bool okt = rowok && (unsigned)tx < (unsigned)W;
            const int base = (row2 * W + tx) * 4;
#pragma unroll
            for (int k = 0; k < KMAX; k += 4) {   // (fully unrolled: Rb stays in registers; groups beyond C are skipped uniformly)
                if (k < nk) {
                    float av[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = 4 * (k + q) + kq;
                        av[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r2, (okt && c < C) ? base + c * HW * 4 : OOBO, 0, 0));
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) accs[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], Rb[k + q], accs[q], 0, 0, 0);
                }
            }
            const corr_v4f acc = (accs[0] + accs[1]) + (accs[2] + accs[3]);
            // lane (n, kq) holds texels m = 4 kq + i of the block for pixel n: offset of the texel from the pixel, in pixels
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int off = 16 * blk + 4 * kq + i - n - md;
                const int q = off / s2;   // (s2 >= 1; exact when the offset is one of the displacements)
                if (off >= -md && off <= md && q * s2 == off) t[(q + r) * 16 + n] = acc[i] * inv;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (wave-local: LDS operations of a wave complete in order)
        float* o = out + ((size_t)b * ND * ND + (size_t)di * ND) * HW + (size_t)y * W + x0;
        for (int idx = lane; idx < ND * 16; idx += 64) {
            const int dj = idx >> 4, px = idx & 15;
            if (x0 + px < W) o[(size_t)dj * HW + px] = t[idx];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

static bool correlation_forward_mfma_ok(int C, int H, int W, int radius, int stride2) {
    return C <= 256 && radius * stride2 <= 16 && (long long)C * H * W * 4 < (1ll << 31);
}

static hipError_t launch_correlation_forward(const float* x1, const float* x2, int B, int C, int H, int W, int radius,
                                             int stride2, float* out, hipStream_t stream) {
    if (radius >= 1 && radius <= RMAX && correlation_forward_mfma_ok(C, H, W, radius, stride2)) {
        const long long nwg = (long long)B * H * ((W + 63) / 64);
        if (nwg < (1ll << 31)) {
            if (C <= 64) hipLaunchKernelGGL((correlation_fwd_mfma_kernel<16>), dim3((unsigned)nwg), dim3(256), 0, stream, x1, x2, C, H, W, radius, stride2, out);
            else if (C <= 128) hipLaunchKernelGGL((correlation_fwd_mfma_kernel<32>), dim3((unsigned)nwg), dim3(256), 0, stream, x1, x2, C, H, W, radius, stride2, out);
            else hipLaunchKernelGGL((correlation_fwd_mfma_kernel<64>), dim3((unsigned)nwg), dim3(256), 0, stream, x1, x2, C, H, W, radius, stride2, out);
            return hipGetLastError();
        }
    }
    const int ND = 2 * radius + 1;
    dim3 grid((W + CT - 1) / CT, (H + CT - 1) / CT, B * ND);
    const size_t lds = correlation_forward_lds(radius, stride2);
    if (lds > CORR_LDS_CAP) return hipErrorInvalidValue;   // (the dispatch never sends such a call here)
    auto go_launch = [&](auto kern) -> hipError_t {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, x1, x2, C, H, W, stride2, out);
        return hipGetLastError();
    };
    switch (radius) {
        case 1: return go_launch(correlation_fwd_kernel<1>);
        case 2: return go_launch(correlation_fwd_kernel<2>);
        case 3: return go_launch(correlation_fwd_kernel<3>);
        case 4: return go_launch(correlation_fwd_kernel<4>);
        default: return hipErrorInvalidValue;
    }
}

// Backward of the correlation: with out[b,d,y,x] = (1/C) sum_c x1[b,c,y,x] * x2[b,c,y+dy,x+dx] (zero padded),
//   grad_x1[b,c,y,x] = (1/C) sum_d go[b,d,y,x]       * x2[b,c,y+dy,x+dx]
//   grad_x2[b,c,y,x] = (1/C) sum_d go[b,d,y-dy,x-dx] * x1[b,c,y-dy,x-dx]
// (correlation_cuda_kernel.cu:116-300 computes the same two sums over its padded NHWC repacks).
// Block = 16x16 pixels x CCH channels: the x1 and x2 halo tiles of the channel chunk are staged in LDS once and
// serve all (2r+1)^2 displacements; a thread reads the two gradient values of a displacement (its own pixel for
// grad_x1, the mirrored pixel for grad_x2) once from global memory and uses them for the CCH channels, so
// the gradient volume is read C/CCH times instead of C times and the features once per tile (+halo) instead of
// (2r+1)^2 times.  Per (pixel, channel) the sum runs over d in ascending order with one fma each, like the
// forward's twin in the oracle.  Launch 1 of the fused cost volume's backward (cost_volume.hip: flow_cost_volume_bwd_kernel)
// restates this loop and store over its own tiles; tests/test_cost_volume_gpu.py holds the two to the same bits.
template <bool WANT1, bool WANT2>
__global__ __launch_bounds__(256) void correlation_bwd_kernel(const float* __restrict__ x1,
                                                              const float* __restrict__ x2,
                                                              const float* __restrict__ go, int C, int H, int W,
                                                              int r, int s2, float* __restrict__ g1,
                                                              float* __restrict__ g2) {
    extern __shared__ float smem[];
    const int halo = r * s2;
    const int TWH = CT + 2 * halo;
    float* t1 = smem;                       // [CCH][TWH][TWH] x1 with halo (for grad_x2)
    float* t2 = smem + CCH * TWH * TWH;     // [CCH][TWH][TWH] x2 with halo (for grad_x1)
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * CT, y0 = blockIdx.y * CT;
    const int c0 = blockIdx.z % ((C + CCH - 1) / CCH) * CCH, b = blockIdx.z / ((C + CCH - 1) / CCH);
    const int x = x0 + tx, y = y0 + ty;
    const int HW = H * W;
    const int nd = 2 * r + 1;
    for (int idx = threadIdx.x; idx < CCH * TWH * TWH; idx += 256) {
        const int cc = idx / (TWH * TWH), rem = idx - cc * TWH * TWH;
        const int ry = rem / TWH, rx = rem - ry * TWH;
        const int gx = x0 - halo + rx, gy = y0 - halo + ry, c = c0 + cc;
        const bool in = c < C && gx >= 0 && gx < W && gy >= 0 && gy < H;
        const size_t off = ((size_t)b * C + c) * HW + gy * W + gx;
        if (WANT2) t1[idx] = in ? x1[off] : 0.0f;
        if (WANT1) t2[idx] = in ? x2[off] : 0.0f;
    }
    __syncthreads();
    const bool inside = x < W && y < H;
    const float* gb = go + (size_t)b * nd * nd * HW;
    float a1[CCH], a2[CCH];
#pragma unroll
    for (int cc = 0; cc < CCH; ++cc) a1[cc] = a2[cc] = 0.0f;
    for (int i = 0; i < nd; ++i) {
        const int dy = (i - r) * s2;
        for (int j = 0; j < nd; ++j) {
            const int dx = (j - r) * s2;
            const float* gd = gb + (size_t)(i * nd + j) * HW;
            if (WANT1) {
                // x2 position paired with (y, x); outside the image the staged tile holds the zeros of the reference's padded
                // buffer and the term is multiplied through like there: +-0 for a finite gradient, NaN for inf or NaN
                const float g = inside ? gd[y * W + x] : 0.0f;
                const float* p = t2 + (ty + halo + dy) * TWH + (tx + halo + dx);
#pragma unroll
                for (int cc = 0; cc < CCH; ++cc) a1[cc] = __builtin_fmaf(g, p[cc * TWH * TWH], a1[cc]);
            }
            if (WANT2) {
                const int ym = y - dy, xm = x - dx;  // x1 position whose pair is (y, x)
                const float g = (inside && ym >= 0 && ym < H && xm >= 0 && xm < W) ? gd[ym * W + xm] : 0.0f;
                const float* p = t1 + (ty + halo - dy) * TWH + (tx + halo - dx);
#pragma unroll
                for (int cc = 0; cc < CCH; ++cc) a2[cc] = __builtin_fmaf(g, p[cc * TWH * TWH], a2[cc]);
            }
        }
    }
    if (!inside) return;
    const float inv = 1.0f / (float)C;
#pragma unroll
    for (int cc = 0; cc < CCH; ++cc) {
        if (c0 + cc >= C) break;
        const size_t o = ((size_t)b * C + c0 + cc) * HW + y * W + x;
        if (WANT1) g1[o] = a1[cc] * inv;
        if (WANT2) g2[o] = a2[cc] * inv;
    }
}

static hipError_t launch_correlation_backward(const float* x1, const float* x2, const float* go, int B, int C, int H, int W,
                                              int radius, int stride2, float* g1, float* g2, hipStream_t stream) {
    const size_t lds = correlation_backward_lds(radius, stride2);
    if (lds > CORR_LDS_CAP) return hipErrorInvalidValue;   // (the dispatch never sends such a call here)
    dim3 grid((W + CT - 1) / CT, (H + CT - 1) / CT, B * ((C + CCH - 1) / CCH));
    auto go_launch = [&](auto kern) -> hipError_t {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, x1, x2, go, C, H, W, radius, stride2, g1, g2);
        return hipGetLastError();
    };
    if (g1 && g2) return go_launch(correlation_bwd_kernel<true, true>);
    if (g1) return go_launch(correlation_bwd_kernel<true, false>);
    if (g2) return go_launch(correlation_bwd_kernel<false, true>);
    return hipSuccess;
}

// ---- the choice of kernel for a call, stated once ---------------------------------------------------------------------------------
using namespace capi;

// kernel_size odd, strides >= 1, and no index of the reference's kernel outside its padded buffers
static int check_corr(const char* who, int32_t B, int32_t C, int32_t H, int32_t W, int32_t pad, int32_t k, int32_t md, int32_t s1, int32_t s2,
                      int* oH, int* oW) {
    if (int rc = check_dims(who, B, C, H, W)) return rc;
    if (pad < 0 || k < 1 || (k & 1) == 0 || md < 0 || s1 < 1 || s2 < 1)
        return fail(PDEPTH_E_ARG, "%s: bad configuration (pad %d, kernel %d, max_displacement %d, stride1 %d, stride2 %d)", who, pad, k, md, s1, s2);
    if (md - (md / s2) * s2 - (k - 1) / 2 < 0)
        return fail(PDEPTH_E_ARG, "%s: kernel_size %d with max_displacement %d / stride2 %d reads outside the padded input in the "
                    "reference kernel (needs (kernel_size-1)/2 <= max_displacement mod stride2)", who, k, md, s2);
    if (!correlation_output_size(H, W, pad, k, md, s1, oH, oW))
        return fail(PDEPTH_E_ARG, "%s: empty output (pad %d too small for max_displacement %d, kernel %d)", who, pad, md, k);
    // (one thread per output / input element in a 1-D grid of 256-thread blocks: below the 2^31 - 1 block limit with room to spare)
    if ((long long)(2 * (md / s2) + 1) * (2 * (md / s2) + 1) * *oH * *oW * B >= (1ll << 38))
        return fail(PDEPTH_E_ARG, "%s: output too large for one launch (2^38 elements)", who);
    if ((long long)B * C * H * W >= (1ll << 38))
        return fail(PDEPTH_E_ARG, "%s: input too large for one launch (2^38 elements)", who);
    return PDEPTH_OK;
}
// the tiled kernels serve fp32 in the configuration of pwclite.py:123-125 and kin ...
static bool corr_fast_path(int half, int32_t pad, int32_t k, int32_t md, int32_t s1, int32_t s2) {
    return !half && k == 1 && s1 == 1 && pad == md && md >= 1 && md % s2 == 0 && md / s2 <= RMAX;
}

// ... as far as their tile fits the LDS (launch_correlation_forward then picks the matrix pipe or the radius); the general kernels
// serve the rest.  half: fp16 I/O.
static int correlation_forward(const char* who, int half, const void* x1, const void* x2, int32_t B, int32_t C, int32_t H, int32_t W,
                               int32_t pad, int32_t k, int32_t md, int32_t s1, int32_t s2, void* out, hipStream_t stream) {
    if (!x1 || !x2 || !out) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    int oH, oW;
    if (int rc = check_corr(who, B, C, H, W, pad, k, md, s1, s2, &oH, &oW)) return rc;
    if (corr_fast_path(half, pad, k, md, s1, s2) && correlation_forward_fits(md / s2, s2))
        return launched(launch_correlation_forward((const float*)x1, (const float*)x2, B, C, H, W, md / s2, s2, (float*)out, stream), who);
    return launched(launch_correlation_general_forward(x1, x2, half, B, C, H, W, pad, k, md, s1, s2, out, stream), who);
}

static int correlation_backward(const char* who, int half, const void* x1, const void* x2, const void* go, int32_t B, int32_t C, int32_t H,
                                int32_t W, int32_t pad, int32_t k, int32_t md, int32_t s1, int32_t s2, void* g1, void* g2, hipStream_t stream) {
    if (!x1 || !x2 || !go || (!g1 && !g2)) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    int oH, oW;
    if (int rc = check_corr(who, B, C, H, W, pad, k, md, s1, s2, &oH, &oW)) return rc;
    if (corr_fast_path(half, pad, k, md, s1, s2) && correlation_backward_fits(md / s2, s2))
        return launched(launch_correlation_backward((const float*)x1, (const float*)x2, (const float*)go, B, C, H, W, md / s2, s2, (float*)g1,
                                                    (float*)g2, stream), who);
    return launched(launch_correlation_general_backward(x1, x2, go, half, B, C, H, W, pad, k, md, s1, s2, g1, g2, stream), who);
}

}  // namespace pdepth

// ---- C ABI (include/pdepth.h; corr_multiply is not read) ----------------------------------------------------------------------------
extern "C" {

int pdepth_correlation_output_size(int32_t H, int32_t W, int32_t pad_size, int32_t kernel_size, int32_t max_displacement, int32_t stride1,
                                   int32_t stride2, int32_t* out_channels, int32_t* out_height, int32_t* out_width) {
    int oH = 0, oW = 0;
    if (int rc = pdepth::check_corr("pdepth_correlation_output_size", 1, 1, H, W, pad_size, kernel_size, max_displacement, stride1, stride2, &oH, &oW))
        return rc;
    if (out_channels) *out_channels = (2 * (max_displacement / stride2) + 1) * (2 * (max_displacement / stride2) + 1);
    if (out_height) *out_height = oH;
    if (out_width) *out_width = oW;
    return PDEPTH_OK;
}

int pdepth_correlation_forward_f32(const float* input1, const float* input2, int32_t B, int32_t C, int32_t H,
                                   int32_t W, int32_t pad_size, int32_t kernel_size, int32_t max_displacement,
                                   int32_t stride1, int32_t stride2, int32_t, float* output, void* stream) {
    return pdepth::correlation_forward("pdepth_correlation_forward_f32", 0, input1, input2, B, C, H, W, pad_size, kernel_size, max_displacement,
                                       stride1, stride2, output, (hipStream_t)stream);
}

int pdepth_correlation_backward_f32(const float* input1, const float* input2, const float* grad_output, int32_t B,
                                    int32_t C, int32_t H, int32_t W, int32_t pad_size, int32_t kernel_size,
                                    int32_t max_displacement, int32_t stride1, int32_t stride2, int32_t,
                                    float* grad_input1, float* grad_input2, void* stream) {
    return pdepth::correlation_backward("pdepth_correlation_backward_f32", 0, input1, input2, grad_output, B, C, H, W, pad_size, kernel_size,
                                        max_displacement, stride1, stride2, grad_input1, grad_input2, (hipStream_t)stream);
}

int pdepth_correlation_forward_f16(const void* input1, const void* input2, int32_t B, int32_t C, int32_t H, int32_t W, int32_t pad_size,
                                   int32_t kernel_size, int32_t max_displacement, int32_t stride1, int32_t stride2,
                                   int32_t, void* output, void* stream) {
    return pdepth::correlation_forward("pdepth_correlation_forward_f16", 1, input1, input2, B, C, H, W, pad_size, kernel_size, max_displacement,
                                       stride1, stride2, output, (hipStream_t)stream);
}

int pdepth_correlation_backward_f16(const void* input1, const void* input2, const void* grad_output, int32_t B, int32_t C, int32_t H,
                                    int32_t W, int32_t pad_size, int32_t kernel_size, int32_t max_displacement, int32_t stride1,
                                    int32_t stride2, int32_t, void* grad_input1, void* grad_input2, void* stream) {
    return pdepth::correlation_backward("pdepth_correlation_backward_f16", 1, input1, input2, grad_output, B, C, H, W, pad_size, kernel_size,
                                        max_displacement, stride1, stride2, grad_input1, grad_input2, (hipStream_t)stream);
}

}  // extern "C"
