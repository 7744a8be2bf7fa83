// The reduction over pixels of the loss terms (loss_terms.hip, loss_smooth1.hip, photo.hip, flow_photo.hip), as loss.hip: every
// workgroup of a launch writes its N partial sums into the workspace, a second launch adds them in a fixed order in double.  No
// atomics: two calls give the same bits.  The workspace holds N planes of one float per workgroup of the first launch, a
// workgroup's slot its index in the grid (x fastest, then y, then z).  Internal linkage: each object that includes this has its
// own copy of what it uses.
#pragma once
#include <hip/hip_runtime.h>

#include "dpv_lanes.hpp"

namespace pdepth {

namespace {

// N planes of `slots` partial sums, to the 256 bytes a workspace is rounded to
inline size_t partial_sums_bytes(int N, size_t slots) { return (N * slots * sizeof(float) + 255) / 256 * 256; }

// N sums of a workgroup -> its slot of each plane
template <int N>
__device__ __forceinline__ void block_partial(const float (&v)[N], float* __restrict__ part) {
    __shared__ float s[N][4];
#pragma unroll
    for (int k = 0; k < N; ++k) wg_sum_put(v[k], s[k]);
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t slots = (size_t)gridDim.x * gridDim.y * gridDim.z;
        const size_t slot = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
#pragma unroll
        for (int k = 0; k < N; ++k) part[k * slots + slot] = wg_sum_get(s[k]);
    }
}

// t[k] = the sum of slots first ... first + n - 1 of plane k (the planes `slots` apart), by one workgroup: thread t adds
// i = t, t + 256, ... in double, then the workgroup's sum.  Every thread returns with the sums.
template <int N>
__device__ __forceinline__ void partial_sums(const float* __restrict__ part, size_t slots, size_t first, int n, float (&t)[N]) {
    __shared__ double s[N][4];
    double a[N];
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] += (double)part[k * slots + first + i];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) wg_sum_put(a[k], s[k]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) t[k] = (float)wg_sum_get(s[k]);
}

// ---- the two partial sums of an item (blockIdx.x) -----------------------------------------------------------------------------------
// MEAN: value = s0 / (mult s1), count = s1 (0 / 0 = NaN for an empty mask).  !MEAN: value = s0 / n0 + s1 / n1.
template <bool MEAN>
__global__ __launch_bounds__(256) void loss_terms_final_kernel(const float* __restrict__ part, int B, int nblk, float n0, float n1,
                                                               float* __restrict__ value, float* __restrict__ count) {
    const int b = blockIdx.x;
    float t[2];
    partial_sums(part, (size_t)B * nblk, (size_t)b * nblk, nblk, t);
    if (threadIdx.x != 0) return;
    if (MEAN) {
        value[b] = t[0] / (n0 * t[1]);
        count[b] = t[1];
    } else {
        value[b] = t[0] / n0 + t[1] / n1;
    }
}

template <bool MEAN>
hipError_t finish(const float* part, int B, int nblk, float n0, float n1, float* value, float* count, hipStream_t stream) {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(loss_terms_final_kernel<MEAN>, dim3(B), dim3(256), 0, stream, part, B, nblk, n0, n1, value, count);
    return hipGetLastError();
}

// of the launches that end in finish(): one workgroup per 256 pixels and item, two sums
inline size_t two_sums_workspace_bytes(int B, int H, int W) { return partial_sums_bytes(2, (size_t)B * n_blocks(H, W)); }

}  // namespace

}  // namespace pdepth
