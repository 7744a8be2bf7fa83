// Wave-level helpers of the persistent sweep kernels: cross-lane scans and reductions, LDS-DMA, packed-fp32 sample
// positions (two planes per instruction, bit-identical to geometry.hpp's scalar chain), the packed cell of a position.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "geometry.hpp"

namespace pdepth {
namespace wv {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int OOB = 0x7fffffff;        // buffer offset beyond every descriptor: the load returns 0
constexpr int NO_CELL = (int)0x80008000u;   // (cell_x, cell_y of it: -32768, -32768 -- neutral in a max)

__device__ __forceinline__ int opaque_v(int x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ int opaque_s(int x) { asm volatile("" : "+s"(x)); return x; }

// workgroup barrier that waits for this wave's LDS traffic only: global loads and stores stay in flight
#define PDEPTH_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// LDS-DMA (buffer_load ... lds): a wave-instruction moves 16 bytes per active lane from memory to LDS address
// m0 + 16 * lane, no registers in between.  Issued from inline asm (the compiler must not know that these loads write LDS,
// or it drains them in front of the next LDS read); counted in vmcnt like every load: the issuing wave waits for them by hand.
template <typename Rsrc>   // (v4i, or the compiler's own __amdgpu_buffer_rsrc_t: the descriptor the builtin loads of the same view use)
__device__ __forceinline__ void dma_b128(Rsrc rsrc, unsigned lds_addr, int voff, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :: "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory", "m0");
}
// ... 4 bytes per active lane, to m0 + 4 * lane (an offset beyond the descriptor writes zero)
template <typename Rsrc>
__device__ __forceinline__ void dma_b32(Rsrc rsrc, unsigned lds_addr, int voff, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds"
                 :: "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory", "m0");
}
__device__ __forceinline__ unsigned lds_addr_of(const void* p) {
    return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void*)p;
}

// inclusive prefix sum over the 64 lanes: Hillis-Steele inside the rows of 16 (DPP row_shr), then the row totals
__device__ __forceinline__ int wave_scan_incl(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
    return v;
}
// min / max over the 64 lanes, the DPP modifier on the min / max itself (the compiler expands update_dpp + min into a move, two
// wait states and the operation per step: 25 instructions per reduction where these take 9); the first step's operand is
// written right in front: a DPP read of a VGPR a vector instruction has just written needs two wait states
#define PDEPTH_WAVE_REDUCE(NAME, OP, SOP)                                                                                  \
    __device__ __forceinline__ int NAME(int v) {                                                                           \
        asm volatile("s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"          \
                     OP " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                        \
                     OP " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                            \
                     OP " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf" : "+v"(v));                                    \
        return SOP(SOP(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),                                 \
                   SOP(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));                               \
    }
PDEPTH_WAVE_REDUCE(wave_min_i, "v_min_i32_dpp", min)
PDEPTH_WAVE_REDUCE(wave_max_i, "v_max_i32_dpp", max)
#undef PDEPTH_WAVE_REDUCE

// CAUTION, packed fp32 (v_pk_mul / v_pk_add / v_pk_fma_f32) on gfx950, ROCm 7.2; measured in sweep_dist.hip with
// plane_sample_pos_fast() of geometry.hpp written for two planes at a time (tools/dbg/dist_dbg.py): in a kernel whose other
// waves run v_mfma_f32_16x16x32_f16 on the same SIMD, these packed instructions now and then leave the LOW half of a result
// unwritten in lanes 48..63 (a sample's position then lacks exactly one operation of the chain: px without K@t, gy without
// the "- cy", ...).  Never in the first pass of a workgroup (every wave of the chip is in its position phase then), on any
// later pass a few hundred samples per launch; a drain of all counters and s_nops in front make no difference, the scalar
// chain of geometry.hpp on the same inputs is always right.  A probe build with two v_mfma_f32_16x16x16_f16 per K = 32 operand
// pair in place of the K = 32 instruction never showed it: the erratum needs v_mfma_f32_16x16x32_f16 in the other waves.
// So no kernel of this library uses packed fp32
// (tests/test_isa_guard.py checks the listing of sweep_dist.hip).

// Footprint of a sample position as make_footprint() (geometry.hpp) computes it, packed: (y0 << 16) | (x0 & 0xffff) of the
// top-left texel, or NO_CELL when no tap lies inside the image (NaN positions included); fw, fn = the fractions.
__device__ __forceinline__ int cell_of(float ix, float iy, int W, int H, float& fw, float& fn) {
    const float xfl = floorf(ix), yfl = floorf(iy);
    fw = ix - xfl;
    fn = iy - yfl;
    // (v_med3_f32: one instruction, no canonicalising v_max in front as fminf / fmaxf get; a NaN comes out as one of the bounds
    //  and is caught by the ordered compare below)
    const int x0 = (int)__builtin_amdgcn_fmed3f(xfl, -2.0f, (float)(W + 1));
    const int y0 = (int)__builtin_amdgcn_fmed3f(yfl, -2.0f, (float)(H + 1));
    const bool any = ix == ix && iy == iy && (unsigned)(x0 + 1) < (unsigned)(W + 1) && (unsigned)(y0 + 1) < (unsigned)(H + 1);
    return any ? (y0 << 16) | (x0 & 0xffff) : NO_CELL;
}
__device__ __forceinline__ int cell_x(int xy) { return (int)(short)(xy & 0xffff); }
__device__ __forceinline__ int cell_y(int xy) { return xy >> 16; }

// x of lane ^ 16 (ds_swizzle: the pattern is part of the instruction) / of the lane whose byte address `a32` holds
// ((lane ^ 32) << 2, computed once): __shfl_xor spends three vector instructions per call on that address
__device__ __forceinline__ float xor16_f(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, x), 0x401f));
}
__device__ __forceinline__ float bperm_f(int a32, float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(a32, __builtin_bit_cast(int, x)));
}
// max without the canonicalising v_max_f32 x, x, x the compiler puts in front of fmaxf (a NaN operand: the other one)
__device__ __forceinline__ float max_raw(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// All-reduce over the four K-slice lanes of a pixel (lanes l, l ^ 16, l ^ 32, l ^ 48): the sum / max_raw of the four values in
// every one of them -- x combined with lane ^ 16's first, the result with lane ^ 32's, this lane's value the first operand both
// times -- by either transport:
//   XCHG == 0  the LDS pipe: ds_swizzle + ds_bpermute (a32 = (lane ^ 32) << 2), an lgkmcnt wait behind each;
//   XCHG == 1  the vector pipe: v_permlane16_swap_b32 exchanges the odd rows of 16 of its first operand with the even rows of
//              its second, v_permlane32_swap_b32 the upper half of the first with the lower half of the second.  On two copies
//              of x one of the two results is, in every lane, its partner's value: the second result in the even rows / the
//              lower half, the first in the others -- picked with a constant lane mask (one v_cndmask, no compare).  No LDS
//              queue, no lgkmcnt; the swaps read copies the compiler makes, and it pads the hazard "vector write -> swap
//              reads it" itself.
// The same bits, NaNs included, as long as the operand order is kept: a + b and b + a differ where both are NaNs of different
// signs (an input NaN beside the -NaN that inf - inf makes; a first form that added the swaps' two results as they came failed
// tools/mb_lane_exchange.hip on exactly that).  That program compares the two transports bit for bit, beside
// v_mfma_f32_16x16x32_f16 and LDS atomics in the other waves of the SIMD as well (the packed-fp32 finding above is why a new
// cross-lane instruction gets that look), and times a step of either: 68 against 32 cycles in a dependent chain.
// sweep_dist.hip uses the LDS pipe all the same (DIST_LANE_XCHG): in that kernel the swaps' copies, picks and pads cost the
// vector pipe what the LDS round trips cost in waiting (profiles/r15_lane_exchange/).
template <int XCHG, bool MAX>
__device__ __forceinline__ float quad_reduce(float x, int a32) {
    auto comb = [](float a, float b) { return MAX ? max_raw(a, b) : a + b; };
    auto f = [](unsigned u) { return __builtin_bit_cast(float, u); };
    static_assert(XCHG == 0 || XCHG == 1, "the transport: 0 = LDS pipe, 1 = lane swaps");
    if (XCHG == 1) {
        const unsigned u = __builtin_bit_cast(unsigned, x);
        const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        x = comb(x, __builtin_amdgcn_inverse_ballot_w64(0xffff0000ffff0000ull) ? f(r[0]) : f(r[1]));
        const unsigned v = __builtin_bit_cast(unsigned, x);
        const auto s = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return comb(x, __builtin_amdgcn_inverse_ballot_w64(0xffffffff00000000ull) ? f(s[0]) : f(s[1]));
    } else {
        x = comb(x, xor16_f(x));
        return comb(x, bperm_f(a32, x));
    }
}
template <int XCHG> __device__ __forceinline__ float quad_sum(float x, int a32) { return quad_reduce<XCHG, false>(x, a32); }
template <int XCHG> __device__ __forceinline__ float quad_max(float x, int a32) { return quad_reduce<XCHG, true>(x, a32); }

template <typename T>
__device__ __forceinline__ T kernarg_at(size_t offset) {
    typedef const char __attribute__((address_space(4))) * kptr;
    typedef const volatile T __attribute__((address_space(4))) * vptr;
    return *(vptr)((kptr)__builtin_amdgcn_kernarg_segment_ptr() + offset);
}

}  // namespace wv
}  // namespace pdepth
