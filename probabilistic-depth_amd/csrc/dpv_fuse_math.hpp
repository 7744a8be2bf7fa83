// exp / log / divide of the DPV fusion kernels (dpv_fuse.hip: forward; dpv_fuse_bwd.hip: backward).  Both include this header, so
// the backward recomputes the forward's values bit for bit and decides the clamp on the number the forward clamped.
// That claim is tested on every pair of forward and backward kernels (tests/test_fuse_gpu.py: test_forward_and_backward_agree_on_q,
// test_forward_and_backward_agree_on_the_clamp).
//
// Hardware exp2 / log2 with an exact-argument reduction (exp_nonpos, geometry.hpp: ~1.5 ulp), log2 x ln 2 (~2 ulp, absolute 1e-7
// near 1) and a refined reciprocal -- the libm forms cost ~20 instructions each, five per element, and made the forward VALU
// bound (127 us for 402 MB).  -DPDEPTH_LIBM_FUSE restores them.
#pragma once
#include <hip/hip_runtime.h>

#include "geometry.hpp"

namespace pdepth {

#ifdef PDEPTH_LIBM_FUSE
__device__ __forceinline__ float fuse_exp(float x) { return expf(x); }
__device__ __forceinline__ float fuse_log(float x) { return logf(x); }
__device__ __forceinline__ float fuse_div(float a, float b, float) { return a / b; }
__device__ __forceinline__ float fuse_rcp(float) { return 0.0f; }
#else
__device__ __forceinline__ float fuse_exp(float x) { return exp_nonpos(x); }
__device__ __forceinline__ float fuse_log(float x) { return __builtin_amdgcn_logf(x) * 0.693147180559945309417f; }
__device__ __forceinline__ float fuse_div(float a, float, float rb) { return a * rb; }
__device__ __forceinline__ float fuse_rcp(float b) { return refined_rcp(b); }
#endif

}  // namespace pdepth
