// The fill in front of every scatter: a destination, an accumulator or a z-buffer set to one 32-bit word by a launch of its own.
//
// A kernel, not hipMemsetAsync.  Eagerly the two are the same.  Captured into a graph they are not: a memset node in front of a
// scatter gave the eager answer on the first replay and another one on a replay with new data in the captured buffers -- for the
// z-buffer of lidar_depth.hip when it was written, and for every memset-fronted path of the library once they
// were replayed (tests/test_graph_replay_gpu.py): values of the previous replay survived in elements the scatter
// did not reach.  A kernel node is ordered like every other launch of the stream.
//
// One launch whatever the size: a thread stores up to FILL_PER_THREAD 16-byte words, a block 16 KB of consecutive addresses (each
// of its stores a full 4 KB row of the block's span); the words in front of the first 16-byte boundary and behind the last are
// stored one by one by the first block.  Every store is guarded by the count it belongs to.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace pdepth {

namespace {

constexpr int FILL_PER_THREAD = 4;
constexpr size_t FILL_PER_BLOCK = 256 * FILL_PER_THREAD;   // 16-byte words

// dst: `head` words (< 4), then n16 16-byte words from the first 16-byte boundary, then `tail` words (< 4)
__global__ __launch_bounds__(256) void fill32_kernel(uint32_t* __restrict__ dst, uint32_t word, unsigned head, size_t n16, unsigned tail) {
    uint4* body = reinterpret_cast<uint4*>(dst + head);
    const size_t first = (size_t)blockIdx.x * FILL_PER_BLOCK + threadIdx.x;
    const uint4 w = make_uint4(word, word, word, word);
#pragma unroll
    for (int k = 0; k < FILL_PER_THREAD; ++k) {
        const size_t i = first + (size_t)k * 256;
        if (i < n16) body[i] = w;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) dst[threadIdx.x] = word;
        if (threadIdx.x < tail) dst[head + 4 * n16 + threadIdx.x] = word;
    }
}

}  // namespace

hipError_t launch_fill32(void* dst, uint32_t word, size_t bytes, hipStream_t stream) {
    if (bytes == 0) return hipSuccess;
    if (!dst || (reinterpret_cast<uintptr_t>(dst) & 3) != 0 || (bytes & 3) != 0) return hipErrorInvalidValue;
    const size_t words = bytes / 4;
    const size_t to_boundary = ((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / 4;
    const unsigned head = (unsigned)(to_boundary < words ? to_boundary : words);
    const size_t n16 = (words - head) / 4;
    const unsigned tail = (unsigned)(words - head - 4 * n16);
    const size_t blocks = n16 ? (n16 + FILL_PER_BLOCK - 1) / FILL_PER_BLOCK : 1;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fill32_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<uint32_t*>(dst), word, head, n16, tail);
    return hipGetLastError();
}

}  // namespace pdepth
