// The workspace of a sweep call (pdepth_sweep_workspace_bytes), described once: its regions, the slots of its 64 queue ints,
// the offsets of a statistics row, and the host-side view the launchers take their pointers from.  Nothing else computes
// an offset into it.
//
//     [tile flags: one int per (batch item, 16x4 tile)]      LDS-tiled kernel: tiles handed to the gather kernel.  The
//         rounded up to 256 bytes (>= 64 ints)               distance-form kernel has no tile flags: it keeps its eight
//                                                            per-XCD queue counters in these ints, up to DIST_QSTRIDE ints
//                                                            apart (SweepWorkspace::dist_queue_counters)
//     [64 queue ints]                                        slots 0-7: per-XCD queue counters of the persistent LDS-tiled
//                                                            kernel; then the slots named below.  50 and 52-55 are reserved
//                                                            and kept zero (retired kernels' slots)
//     [packed source]                                        the larger of the two staging layouts, so that one size serves
//                                                            both kernel families:
//         B*V x (ceil(C/4) + 2) x H x W float4               channel-group-planar (sweep_pack.hip): planes g < ceil(C/4) hold
//                                                            channels 4g..4g+3 of every texel, minus mu[c]; then the two
//                                                            Gram planes
//         B*V x dist::view_bytes(C, H, W), to 256 bytes      distance form (dist_layout.hpp), C <= 72 only
//     [reserved: as many bytes as the tile flags]            a retired kernel's tile list.  Nothing reads or writes it; it stays
//                                                            so that the statistics are where a workspace packed by an
//                                                            earlier build of ABI 6 has them
//     [statistics: B x STATS_STRIDE floats, to 256 bytes]    per batch item: mu[c] (the constant subtracted per channel; zeros =
//                                                            not centred) at +0, var[c] at +STATS_VAR, ... (below)
//
// Mean-centring: mu[b][c] = mean of channel c over a sample of 8 rows of source view 0 of item b -- an estimate is all it
// takes, what matters is that the residual offset is small against the spread.  The distance-form layout is centred
// (pack_dist.hip reads these statistics).  The channel-group-planar layout is not (the LDS-tiled kernel: direct form on the
// near planes): mu = 0, and the pre-pass raises NONCENTRED_SLOT when the squared channel offsets exceed half the summed
// variances; the tiled kernel then evaluates every plane directly.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "dist_layout.hpp"
#include "kernels.hpp"

namespace pdepth {

// the 64 workspace ints behind the tile flags.  Slots 50 and 52-55 are reserved and kept zero (they belonged to retired kernels;
// the pack kernels and the flag clear zero them with the rest), so a workspace packed by an earlier build of ABI 6 stays valid.
constexpr int QUEUE_INTS = 64;
// counter of the tiles handed to the gather kernel: every writer of a gather flag increments it, the gather kernel's blocks
// leave at once while it is zero
constexpr int GATHER_COUNT_SLOT = 48;
constexpr int NONCENTRED_SLOT = 51;        // set by the pre-pass of a NOT centred source whose channel offsets exceed the spread (sweep_pack.hip)
// which staging layout the packed-source region holds (written by the pack kernels, checked by the sweep kernels: a sweep on
// another family's layout fills its outputs with NaN instead of returning numbers computed from the wrong bytes)
constexpr int LAYOUT_SLOT = 56;
constexpr int LAYOUT_C4 = 1, LAYOUT_DIST16 = 3;   // (0: nothing packed yet; 2: reserved, a retired layout)
// sweep_dist.hip: workgroups that have left (the last one zeroes the queue counters); pixel blocks evaluated directly, this call
// so far / of the last finished call
constexpr int DIST_DONE_SLOT = 57, DIST_DIRECT_SLOT = 58, DIST_DIRECT_LAST_SLOT = 59;
// DIST_DIRECT_LAST_SLOT holds (nonce << 20) | count, DIST_NONCE_SLOT the nonce of the last call: a count whose nonce is another
// call's reads as 0 (where every workgroup runs one item there is no counter of finished workgroups to reset anything by: 2 048
// returning atomics on one address were a quarter of such a launch)
constexpr int DIST_NONCE_SLOT = 60;

// channel statistics of the source (sweep_pack.hip): per batch item mu[c] at +0, var[c] at +STATS_VAR, the
// squared offset that was NOT subtracted at +STATS_OFF, the largest sampled |x| at +STATS_AMAX, half the mean squared
// difference of samples STATS_LAG_PX texels apart at +STATS_LAG (the spread of a channel at the distance of a plane sweep:
// equal to var[c] for white features, smaller for smooth ones), and STATS_NFLAG ints at +STATS_FLAGS: [1] != 0 = the item was left to the gather kernel (sweep_dist.hip: routing); [0] != 0 = a feature
// of the item did not fit the fp16 range of the distance-form layout (pack_dist.hip)
constexpr int STATS_VAR = 80, STATS_OFF = 160, STATS_AMAX = 240, STATS_LAG = 320, STATS_FLAGS = 400, STATS_NFLAG = 16, STATS_STRIDE = 496;
// (the 80 ints at +416 of a row are reserved: a retired pre-pass kept per-channel tags there; the stride is what ABI 6 callers sized
// their workspaces by)
constexpr int STATS_LAG_PX = 16;

// byte offsets of the regions from the workspace's base (the tile flags are at 0), and the size of the whole
struct SweepWorkspaceOffsets {
    size_t queue, packed, stats, total;
};
inline SweepWorkspaceOffsets sweep_workspace_offsets(int B, int V, int C, int H, int W) {
    const auto to256 = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t tiles = (size_t)((W + 15) / 16) * ((H + 3) / 4);
    const size_t flags = to256((size_t)B * tiles * sizeof(int));
    const size_t c4 = (size_t)B * V * ((C + 3) / 4 + 2) * H * W * 16;
    const size_t d16 = C <= dist::MAX_C ? to256((size_t)B * V * (size_t)dist::view_bytes(C, H, W)) : 0;
    SweepWorkspaceOffsets o;
    o.queue = flags;
    o.packed = flags + QUEUE_INTS * sizeof(int);
    o.stats = o.packed + (c4 > d16 ? c4 : d16) + flags;   // (+ flags: the reserved region)
    o.total = o.stats + to256((size_t)B * STATS_STRIDE * sizeof(float));
    return o;
}
// what pdepth_sweep_workspace_bytes answers, for the LDS-tiled and the distance-form kernel alike
inline size_t sweep_workspace_bytes(int B, int V, int C, int H, int W) { return sweep_workspace_offsets(B, V, C, H, W).total; }

// the regions of one workspace as pointers: what every launcher of a packed-source kernel starts from
struct SweepWorkspace {
    int* flags;     // tile flags
    int nflags;     // ints of the tile-flag region (its 256-byte rounding included: >= 64)
    int* queue;     // the QUEUE_INTS ints behind them
    char* packed;   // packed source, in the layout LAYOUT_SLOT names
    float* stats;   // B rows of STATS_STRIDE floats

    static SweepWorkspace of(void* base, const SweepArgs& a) {
        const SweepWorkspaceOffsets o = sweep_workspace_offsets(a.B, a.V, a.C, a.H, a.W);
        char* p = static_cast<char*>(base);
        return {reinterpret_cast<int*>(p), (int)(o.queue / sizeof(int)), reinterpret_cast<int*>(p + o.queue), p + o.packed,
                reinterpret_cast<float*>(p + o.stats)};
    }
    // the distance-form kernel's queue counters live in the tile-flag ints, which that kernel family does not use otherwise
    int* dist_queue_counters() const { return flags; }
};

// First statement of a sweep kernel on a packed source: does the workspace hold the layout this kernel reads?  If not (a C
// caller swept a workspace packed for another kernel family: include/pdepth.h, pdepth_sweep_source_layout) every output of
// the call is filled with NaN by the whole grid and the kernel leaves: loud numbers instead of costs computed from the
// wrong bytes.  (The packing entry points write the tag; the Python binding refuses the mismatch before it gets here.)
__device__ __forceinline__ bool poison_on_foreign_layout(const SweepArgs& a, const int* __restrict__ queue, int expected) {
    if (queue[LAYOUT_SLOT] == expected) return false;
    const float nan = __builtin_nanf("");
    const size_t hw = (size_t)a.H * a.W, nvol = (size_t)a.B * a.D * hw, nmap = (size_t)a.B * hw;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = i0; i < nvol; i += step) {
        if (a.cost_out) a.cost_out[i] = nan;
        if (a.logp_out) a.logp_out[i] = nan;
    }
    if (a.depth_out)
        for (size_t i = i0; i < nmap; i += step) a.depth_out[i] = nan;
    return true;
}

}  // namespace pdepth
