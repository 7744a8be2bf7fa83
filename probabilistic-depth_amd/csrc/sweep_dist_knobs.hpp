// Build-time knobs of sweep_dist.hip (tools/variants_dist.sh sets them with -D for A/B builds; the defaults are the product).
#pragma once

#ifndef DIST_MAXB1
#define DIST_MAXB1 24      // blocks of 16 texels a pass can take, D <= 64: the most that leaves FOUR workgroups per CU (38 KB of LDS; round 5: 34 at three)
#endif
#ifndef DIST_MAXB2
#define DIST_MAXB2 34      // ... D > 64 (the most that leaves three workgroups per CU: 35 -> two; config 5: 32 -> 34 = 6 809 -> 1 482 direct passes, 5.58 -> 5.03 ms per call)
#endif
#ifndef DIST_OCC1
#define DIST_OCC1 4        // minimum waves per SIMD asked of the compiler at D <= 64: 128 registers (one texel operand set), four workgroups per CU:
#endif                     //    0.332 -> 0.307 ms against three workgroups with two operand sets (profiles/r06_ab/)
#ifndef DIST_OCC2
#define DIST_OCC2 3        // ... at D > 64: without the bound the allocator takes 170 registers (two workgroups per CU: config 5 20 % slower),
#endif                     //    with it 165, nothing spilled
#ifndef DIST_SETS1
#define DIST_SETS1 1       // texel operand register sets of a wave (= its blocks in flight) at D <= 64 (2 at three workgroups per CU: 4 % faster than 1 there, 7 % slower than 1 at four) ...
#endif
#ifndef DIST_SETS2
#define DIST_SETS2 2       // ... and at D > 64 (168 registers under the launch bound, 8 of them spilled: config 5 3.89 -> 3.51 ms all the same)
#endif
#ifndef DIST_BV_LDS
#define DIST_BV_LDS 0      // 1: the pixel-side operands are read from LDS in front of every block's multiplications instead of once per pass
#endif
#ifndef DIST_YSKEW
#define DIST_YSKEW 0       // floats by which the Y rows of pixels 8 .. 15 are shifted (a multiple of 4; 8 = a quarter of the banks)
#endif
#ifndef DIST_XPRIO
#define DIST_XPRIO 1       // wave priority in the matrix phase
#endif
#ifndef DIST_STORE_AUX
#define DIST_STORE_AUX 0   // cache policy of the output stores: default (write-back: the two 32-byte halves of a 64-byte piece, written by the workgroups of neighbouring pixel blocks, merge in L2 -- WRITE_SIZE 145 MB per launch = the output; nt, round 5: 245 MB; same time)
#endif
#ifndef DIST_BANDS
#define DIST_BANDS 16      // bands of tile rows per image in the XCD partition: 16 (XCD q: half-bands q and 8 + q) | 8 (band q: 7 % fewer L2 misses, 5 % slower -- the XCDs' loads differ; profiles/r05_ab/xcd_bands_8_vs_16.txt)
#endif
#ifndef DIST_COL_ALT
#define DIST_COL_ALT 0     // columns of a band from both image borders inwards (1) | left to right (0: 1.2 % faster on the forward motion, 5 % fewer L2 misses)
#endif
#ifndef DIST_QSTRIDE
#define DIST_QSTRIDE 64    // ints between the queue counters of two XCDs (1 -- all eight on one line, round 5 --: memory-side atomics on one line are served one by one, ~13 ns each)
#endif
#ifndef DIST_PREFETCH
#define DIST_PREFETCH 0    // 1: the next pixel block's rays and reference features moved to LDS by LDS-DMA behind the last barrier of the current
#endif                     //    one (bit-identical; headline 0.389 -> 0.407 ms: the second decode and the DMA issue cost more than the wait they hide;
                           //    profiles/r07_ab/)
#ifndef DIST_ABL
#define DIST_ABL 0         // timing only (wrong results), bits: 1 = every sample position computed twice, 2 = no texel loads,
#endif                     //    4 = no pixel loads (rays from a linear fit of batch item 0's, reference features from LDS constants)
#ifndef DIST_ABL_NOB3
#define DIST_ABL_NOB3 0    // timing only (wrong results): no barrier in front of the merge of the waves' softmax parts
#endif
// channel groups of the direct evaluation whose taps are in flight together (3 / 9: 168 registers under a launch bound of 3
// waves per SIMD, no scratch -- and config 5, 1.3 % of whose passes go this way, 8 % slower)
#ifndef DIST_DIRECT_UNROLL
#define DIST_DIRECT_UNROLL 1
#endif
#ifndef DIST_STAGGER
#define DIST_STAGGER 0       // start-up stagger of the persistent workgroups, in sleeps of 6 400 cycles per CU slot (round 5: 2; with single pixel blocks as items the workgroups drift apart within a pass: 0 is as fast on the headline, 5 % faster at B = 1)
#endif
#ifndef DIST_ONE_EACH_X
// no queue -- a workgroup per item (pixel block), the hardware's dispatcher instead of the per-XCD counters -- up to this many items
// per resident workgroup (2 / 6 / 12 / 24: the headline and config 5 are indifferent; B = 1 256x512 -- 10.7 items per workgroup --
// 94 us persistent, 114 us with a workgroup per item: profiles/r06_ab/)
#define DIST_ONE_EACH_X 6
#endif
#ifndef DIST_GUARD_RATIO
#define DIST_GUARD_RATIO 1.7f   // the guard: energy of the centred features / their spread at a lag of 16 texels, and ...
#endif
#ifndef DIST_GUARD_ENERGY
#define DIST_GUARD_ENERGY 110.0f   // ... energy x 10 / sigma beyond which an item is evaluated directly (sweep_dist.hip)
#endif
#ifndef DIST_EXACT_EXP
#define DIST_EXACT_EXP 0   // 1: geometry.hpp's exp_nonpos (1.5 ulp, 12 instructions) instead of the hardware 2^x on the rounded product
#endif
#ifndef DIST_FORCE_DIRECT
#define DIST_FORCE_DIRECT -2   // test builds: -1 = every pass takes the direct evaluation, v >= 0 = the passes of view v
#endif

// The matrix instruction.  DIST_MFMA16: two K = 16 instructions (v_mfma_f32_16x16x16_f16) per K = 32 operand pair -- the probe
// that showed the packed-fp32 erratum (wave_util.hpp) to need v_mfma_f32_16x16x32_f16 in the other waves.
#ifdef DIST_MFMA16
#define DIST_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_shufflevector(a, a, 4, 5, 6, 7), __builtin_shufflevector(b, b, 4, 5, 6, 7), \
                               __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_shufflevector(a, a, 0, 1, 2, 3), __builtin_shufflevector(b, b, 0, 1, 2, 3), c, 0, 0, 0), 0, 0, 0)
#else
#define DIST_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#endif

// phase stamps (-DDIST_STAMPS): shader-clock cycles per phase, summed per wave, added into the queue ints 8..31 on the way out
// (every stamp is a scalar memory read and a wait for it: the phases stretch, their proportions are indicative only)
#ifdef DIST_STAMPS
#define DSTAMP(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); stamp_acc[i] += t_ - stamp_t; stamp_t = t_; }
#elif defined(DIST_MARKS)   // static instruction census per phase (tools/dbg/isa_census.py)
#define DSTAMP(i) asm volatile("; MARK " #i ::: "memory");
#else
#define DSTAMP(i)
#endif
