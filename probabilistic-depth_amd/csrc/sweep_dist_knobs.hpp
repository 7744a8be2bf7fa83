// Build-time knobs of sweep_dist.hip: the defaults are the product; tools/variants_dist.sh builds a library with other values
// (-D).  What the retired knobs measured is in DESIGN.md and profiles/r0*_ab/.
#pragma once

#ifndef DIST_MAXB1
#define DIST_MAXB1 24      // blocks of 16 texels a pass can take at D <= 64: the most that leaves four workgroups per CU (38 KB of LDS)
#endif
#ifndef DIST_MAXB2
#define DIST_MAXB2 34      // ... at D > 64: the most that leaves three workgroups per CU (config 5: 32 -> 34 = 6 809 -> 1 482 direct passes)
#endif
#ifndef DIST_OCC1
#define DIST_OCC1 4        // minimum waves per SIMD asked of the compiler at D <= 64: 128 registers, four workgroups per CU (0.332 -> 0.307 ms against three)
#endif
#ifndef DIST_OCC2
#define DIST_OCC2 3        // ... at D > 64: without the bound the allocator takes 170 registers (two workgroups per CU: config 5 20 % slower)
#endif
#ifndef DIST_SETS1
#define DIST_SETS1 1       // texel operand register sets of a wave (= its blocks in flight) at D <= 64: 2 is 7 % slower at four workgroups per CU
#endif
#ifndef DIST_SETS2
#define DIST_SETS2 2       // ... at D > 64: 165 registers under the launch bound, nothing spilled, config 5 3.89 -> 3.51 ms against 1
#endif
#ifndef DIST_QSTRIDE
#define DIST_QSTRIDE 64    // ints between the queue counters of two XCDs: memory-side atomics on one line are served one by one, ~13 ns each
#endif
#ifndef DIST_PREFETCH
#define DIST_PREFETCH 0    // 1: the next pixel block's rays and reference features by LDS-DMA behind the current one's last barrier (bit-identical; 1.6 % slower on the item record, 5 % before it: profiles/r10_item_record/, r07_ab/)
#endif
#ifndef DIST_DECODE_EARLY
#define DIST_DECODE_EARLY 2   // where the queue thread decodes the next item and pops the one after it: 2 = in the item's first pass, behind its wave's last texel block (the other waves still multiply); 1 = at the top of the block, under its pixel loads (the other waves wait at the first barrier: +2.1 % headline); 0 = in front of the block's last barrier (+2.3 %): profiles/r13_wave_roles/, r10_item_record/
#endif
#ifndef DIST_QUEUE_WAVE
#define DIST_QUEUE_WAVE 3     // the wave whose lane 0 is the workgroup's queue thread (pops, resolves, decodes, publishes, counts, leaves); with DIST_DECODE_EARLY == 2 the last wave in the order of the texel-block shares, whichever it is (wave 0 there, with its full share: +2.2 % headline)
#endif
#ifndef DIST_REV_BATCH
#define DIST_REV_BATCH 1      // 1: on the NCHW entry the queues hand out the batch items last to first -- the pack kernel wrote the last one last (bit-identical; headline -2.1 %, the sweep kernel 277 -> 272 us: profiles/r14_l2_warm/); 0: first to last
#endif
#ifndef DIST_LANE_XCHG
#define DIST_LANE_XCHG 0      // how the centring's and the partial softmax's sums and maxima cross the four K-slice lanes of a pixel (wave_util.hpp: quad_sum, quad_max): 0 = ds_swizzle + ds_bpermute (LDS pipe, an lgkmcnt wait behind each); 1 = v_permlane16_swap / v_permlane32_swap (vector pipe; bit-identical; headline +0.4 us alone, +1.7 us beside DIST_ROWTAB_FOLD: profiles/r15_lane_exchange/)
#endif
#ifndef DIST_ROWTAB_FOLD
#define DIST_ROWTAB_FOLD 1    // 1: the row table's last update of a thread is folded over groups of eight lanes with DPP where they end on one row, one lane issuing the two LDS atomics (bit-identical; headline -1.3 %, --pose stereo -7.1 %, config 5 -2.1 %: profiles/r15_lane_exchange/); 0: every lane issues its own
#endif
#ifndef DIST_ONE_EACH_X
#define DIST_ONE_EACH_X 6  // a workgroup per item, no queue, up to this many items per resident workgroup (2 .. 24: the large shapes are indifferent; profiles/r06_ab/)
#endif
#ifndef DIST_GUARD_RATIO
#define DIST_GUARD_RATIO 1.7f   // the guard: energy of the centred features / their spread at a lag of 16 texels, and ...
#endif
#ifndef DIST_GUARD_ENERGY
#define DIST_GUARD_ENERGY 110.0f   // ... energy x 10 / sigma beyond which an item is evaluated directly (sweep_dist.hip: "Guard" says how both were calibrated)
#endif
#ifndef DIST_FORCE_DIRECT
#define DIST_FORCE_DIRECT -2   // test builds: -1 = every pass takes the direct evaluation, v >= 0 = the passes of view v
#endif

// phase stamps (-DDIST_STAMPS): shader-clock cycles per phase, summed per wave, added into the queue ints 8..31 on the way out
// (every stamp is a scalar memory read and a wait for it: the phases stretch, their proportions are indicative only).
// -DDIST_STAMP_WAVE=w: only wave w of every workgroup reports (four builds, four runs: tools/dbg/dist_stamps.py --libs puts
// them side by side) -- the wave whose barrier stamp is near zero is the one the other three waited for
#ifndef DIST_STAMP_WAVE
#define DIST_STAMP_WAVE -1
#endif
#ifdef DIST_STAMPS
#define DSTAMP(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); stamp_acc[i] += t_ - stamp_t; stamp_t = t_; }
#elif defined(DIST_MARKS)   // static instruction census per phase (tools/dbg/isa_census.py)
#define DSTAMP(i) asm volatile("; MARK " #i ::: "memory");
#else
#define DSTAMP(i)
#endif
