// The pixel reduction of the loss terms (loss_terms.hip, loss_smooth1.hip), as loss.hip: a workgroup (256 pixels) writes two
// partial sums into the workspace, a second launch of one workgroup per item adds them in a fixed order in double.  No atomics: two
// calls give the same bits.  Internal linkage: each object that includes this has its own copy of the final kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "dpv_lanes.hpp"

namespace pdepth {

namespace {

// two sums of a workgroup -> its slots of the workspace ([2][B][nblk])
__device__ __forceinline__ void block_partial(float s0, float s1, float* __restrict__ part, int nitems) {
    __shared__ float sa[4];
    __shared__ float sb[4];
    wg_sum_put(s0, sa);
    wg_sum_put(s1, sb);
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[slot] = wg_sum_get(sa);
        part[(size_t)nitems * gridDim.x + slot] = wg_sum_get(sb);
    }
}

// ---- the partial sums of an item in a fixed order ----------------------------------------------------------------------------------
// MEAN: value = s0 / (mult s1), count = s1 (0 / 0 = NaN for an empty mask).  !MEAN: value = s0 / n0 + s1 / n1.
template <bool MEAN>
__global__ __launch_bounds__(256) void loss_terms_final_kernel(const float* __restrict__ part, int B, int nblk, float n0, float n1,
                                                               float* __restrict__ value, float* __restrict__ count) {
    __shared__ double sa[4];
    __shared__ double sb[4];
    const int b = blockIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) {
        s0 += (double)part[(size_t)b * nblk + i];
        s1 += (double)part[((size_t)B + b) * nblk + i];
    }
    wg_sum_put(s0, sa);
    wg_sum_put(s1, sb);
    __syncthreads();
    if (threadIdx.x == 0) {
        const float t0 = (float)wg_sum_get(sa), t1 = (float)wg_sum_get(sb);
        if (MEAN) {
            value[b] = t0 / (n0 * t1);
            count[b] = t1;
        } else {
            value[b] = t0 / n0 + t1 / n1;
        }
    }
}

template <bool MEAN>
hipError_t finish(const float* part, int B, int nblk, float n0, float n1, float* value, float* count, hipStream_t stream) {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(loss_terms_final_kernel<MEAN>, dim3(B), dim3(256), 0, stream, part, B, nblk, n0, n1, value, count);
    return hipGetLastError();
}

size_t workspace_bytes(int B, int H, int W) { return ((size_t)2 * B * n_blocks(H, W) * sizeof(float) + 255) / 256 * 256; }

}  // namespace

}  // namespace pdepth
