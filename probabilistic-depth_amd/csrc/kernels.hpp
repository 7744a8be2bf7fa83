// Internal launch interface between translation units: what the C ABI of capi.hip launches, and what one kernel file calls of another.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace pdepth {

// Flattened arguments of one sweep launch (device pointers, element strides).
struct SweepArgs {
    const float* ref;
    const float* src;
    const float* K;
    const float* R;
    const float* t;
    const float* rays;
    const float* cxcy;
    const float* d_candi;
    float* cost_out;   // [B,D,H,W] or nullptr
    float* logp_out;   // [B,D,H,W] or nullptr
    float* depth_out;  // [B,H,W]   or nullptr
    int B, V, C, D, H, W;
    int metric;
    int blas_mode;
    int fast_div;      // 1: shared-reciprocal divide chain (geometry.hpp), 0: compiler's IEEE divides
    float sigma;
    long long ref_bstride, src_bstride, src_vstride;
    // the source views in the sweep kernels' staging layout ([B*V][C/4 + 2][H][W] float4, sweep_tiled.hip), set by the
    // launcher of the tiled path: the gather kernel reads it for the tiles handed to it when src == nullptr
    // (packed-source entry: the caller no longer has the NCHW source)
    const void* packed_src;
};
// conditioning above which a batch item is routed to the gather kernel (sweep_dist.hip: "Conditioning"; sweep_pack.hip)
#ifndef PDEPTH_COND_LIMIT
#define PDEPTH_COND_LIMIT 4.0e-4f
#endif
// ... for the LDS-tiled kernel, whose correlation-form plane group is noisier than the distance form (soak 9107: 1.04e-4 /
// 1.09e-4 m, scaled, at 2.0e-4 / 2.3e-4 of this measure on unit-variance features, V = 3)
#ifndef PDEPTH_COND_LIMIT_TILED
#define PDEPTH_COND_LIMIT_TILED 1.5e-4f
#endif
// sweep_direct.hip
hipError_t launch_sweep_direct(const SweepArgs& a, hipStream_t stream);
// the tiles whose flag == flag_value; gather_count: the workspace's GATHER_COUNT_SLOT (sweep_workspace.hpp)
hipError_t launch_sweep_direct_flagged(const SweepArgs& a, const int* tile_flags, const int* gather_count, int tiles_x,
                                       int tiles, hipStream_t stream, int flag_value = 1);
// ... the whole batch items b with item_flags[b * item_stride] != 0 (the distance-form kernel's routed items: STATS_FLAGS + 1)
hipError_t launch_sweep_direct_items(const SweepArgs& a, const int* item_flags, int item_stride, hipStream_t stream);
int sweep_direct_max_planes(int C);

// sweep_tiled.hip (the workspace of every launcher below that takes one: sweep_workspace.hpp)
int sweep_tiled_max_planes();
// packed_ready: the workspace already holds the packed source of exactly these views (pdepth_pack_source_f32)
hipError_t launch_sweep_tiled(const SweepArgs& a, void* workspace, hipStream_t stream, bool packed_ready = false);     // picks a variant
hipError_t launch_sweep_tiled_n1(const SweepArgs& a, void* workspace, hipStream_t stream, bool packed_ready = false);  // one 16x4 tile per block
hipError_t launch_sweep_tiled_n2(const SweepArgs& a, void* workspace, hipStream_t stream, bool packed_ready = false);  // two tiles per block

// sweep_pack.hip: pre-pass of the packed-source kernels (channel statistics + packed source + Gram planes; clears flags and
// queue counters) in the plain layout (nothing subtracted: mu = 0)
hipError_t launch_pack_c4(const SweepArgs& a, void* workspace, hipStream_t stream);
hipError_t clear_sweep_flags(const SweepArgs& a, void* workspace, hipStream_t stream);
// encoder epilogue: cat(feat, avg_pool2d(rgb)) -> packed source views + NCHW reference view, in one pass (a.C = Cf + 3)
hipError_t launch_pack_views(const SweepArgs& a, const float* feat, const float* rgb, int rate, int img_h, int img_w, float* ref_out,
                             void* workspace, hipStream_t stream);
int sweep_device_cus();

// sweep_pack.hip: the channel statistics alone (mean-centring on), for the pack kernels of pack_dist.hip
hipError_t launch_feature_stats(const SweepArgs& a, float* stats, hipStream_t stream);
int sweep_resident_workgroups();   // 256-thread workgroups the device certainly holds at once (conservative)
hipError_t launch_view_stats(const SweepArgs& a, const float* feat, const float* rgb, int rate, int img_h, int img_w, float* stats, hipStream_t stream);
// pack_dist.hip: the statistics kernel, then the source views in the distance-form kernel's layout (dist_layout.hpp)
hipError_t launch_pack_dist(const SweepArgs& a, void* workspace, hipStream_t stream);
hipError_t launch_pack_views_dist(const SweepArgs& a, const float* feat, const float* rgb, int rate, int img_h, int img_w, float* ref_out,
                                  void* workspace, hipStream_t stream);
// sweep_dist.hip (L2 only): distance form sum_t w_t |s_t - r|^2 - Q on the matrix pipe (fp16 high / low parts), C <= 72, D <= 128
bool sweep_dist_supports(const SweepArgs& a);
hipError_t launch_sweep_dist(const SweepArgs& a, void* workspace, hipStream_t stream, bool packed_ready = false);

// dpv.hip
hipError_t launch_dpv_reduce(const float* logits, const float* d_candi, int B, int D, int H,
                             int W, float* logp, float* depth, hipStream_t stream);
hipError_t launch_dpv_reduce_ex(const float* logits, const float* addend, const float* d_candi, int B, int D, int H, int W,
                                float* logp, float* prob, float* depth, float* variance, float* quarter, hipStream_t stream);
hipError_t launch_dpv_expect(const float* dpv, const float* d_candi, int B, int D, int H, int W,
                             int bv_log, float* depth, hipStream_t stream);

// dpv_bwd.hip: gradients of the reductions above with respect to their volume input (any of g_logp / g_prob / g_depth may be
// nullptr, not all)
hipError_t launch_dpv_reduce_backward(const float* logp, const float* d_candi, int B, int D, int H, int W, const float* g_logp,
                                      const float* g_prob, const float* g_depth, float* g_logits, hipStream_t stream);
hipError_t launch_dpv_expect_backward(const float* dpv, const float* d_candi, int B, int D, int H, int W, int bv_log,
                                      const float* g_depth, float* g_dpv, hipStream_t stream);

// dpv_fuse_bwd.hip: gradient of launch_dpv_fuse (dpv_fuse.hip) with respect to logp, recomputed from the forward's inputs; g_fused
// (into fused) / g_logfused (into logfused) may be nullptr, not both
hipError_t launch_dpv_fuse_backward(const float* logp, const float* dmaps, const float* masks, const float* d_candi,
                                    const float* g_fused, const float* g_logfused, int B, int D, int H, int W, float var, float eps,
                                    float* g_logp, hipStream_t stream);

// capi.hip: sets the message pdepth_last_error() returns on this thread, returns code
int api_error(int code, const char* msg);

// loss.hip: soft-label cross-entropy (+ expectation) of a log-DPV, forward and backward.  Exactly one of label [B,D,H,W] /
// depth_gt [B,H,W] is non-null; mask, depth, g_loss, g_depth may be nullptr
size_t dpv_soft_ce_workspace_bytes(int B, int H, int W);
hipError_t launch_dpv_soft_ce(const float* logp, const float* d_candi, const float* label, const float* depth_gt, float variance,
                              float pw, const float* mask, int B, int D, int H, int W, float* loss, float* count, float* depth,
                              void* workspace, hipStream_t stream);
hipError_t launch_dpv_soft_ce_backward(const float* logp, const float* d_candi, const float* label, const float* depth_gt,
                                       float variance, float pw, const float* mask, const float* count, int B, int D, int H, int W,
                                       const float* g_loss, const float* g_depth, float* g_logp, hipStream_t stream);

// metrics.hip: the devkit's nine depth errors per item of a batch.  Exactly one of logp [B,D,H,W] / pred [B,H,W] is non-null;
// mask and depth may be nullptr, clamp_max <= 0 = no clamp
size_t depth_metrics_workspace_bytes(int B, int H, int W);
hipError_t launch_depth_metrics(const float* logp, const float* pred, const float* d_candi, const float* truth, const float* mask,
                                float clamp_max, int B, int D, int H, int W, float* metrics, float* count, float* depth,
                                void* workspace, hipStream_t stream);

// flow_metrics.hip: the flow evaluation per item of a batch (end-point error means, outlier rates, mask sums) of pred [B,2,h,w]
// rescaled and resized to gt [B,gt_channels,H,W]; move_mask [B,H,W] and flow_up [B,2,H,W] may be nullptr.  launch_flow_resize:
// the rescale and resize alone, half-pixel centres or align_corners
size_t flow_metrics_workspace_bytes(int B, int H, int W);
hipError_t launch_flow_metrics(const float* gt, int gt_channels, const float* pred, int h, int w, const float* move_mask, int B, int H,
                               int W, float* errors, float* counts, float* flow_up, void* workspace, hipStream_t stream);
hipError_t launch_flow_resize(const float* flow, int B, int h, int w, int H, int W, bool align_corners, float* out, hipStream_t stream);

// clear.hip: dst[0, bytes) set to one 32-bit word by one launch on the stream (dst 4-byte aligned, bytes a multiple of 4; 16-byte
// stores between the 16-byte boundaries, single words outside them).  What clears a scatter's destination, an integer-sum workspace
// or a z-buffer: a kernel, because a hipMemsetAsync in front of a scatter does not survive a graph replay on new data (clear.hip)
hipError_t launch_fill32(void* dst, uint32_t word, size_t bytes, hipStream_t stream);
inline hipError_t launch_zero(void* dst, size_t bytes, hipStream_t stream) { return launch_fill32(dst, 0u, bytes, stream); }

// lidar_depth.hip: LiDAR scans -> z-buffered, filtered depth maps and masks at full and quarter resolution.  points [B,Nmax,dim]
// (dim 3: w = 1), counts [B], M [4,4] | [B,4,4], intr [3,4] | [B,3,4]; the workspace is the z-buffer
size_t lidar_depth_workspace_bytes(int B, int H, int W);
hipError_t launch_lidar_depth(const float* points, const int* counts, const float* M, const float* intr, int B, int Nmax,
                              int point_dim, int M_batched, int intr_batched, int H, int W, int filtering, float filterdiff,
                              float pool_default, float* dmap, float* mask, float* dmap_q, float* mask_q, void* workspace,
                              hipStream_t stream);

// sweep_bwd.hip: gradient of the cost volume with respect to the NCHW features (either output may be nullptr, not both;
// grad_src [B,V,C,H,W] contiguous, zeroed by the launcher; grad_ref [B,C,H,W] contiguous)
hipError_t launch_sweep_backward(const SweepArgs& a, const float* grad_cost, float* grad_ref, float* grad_src, hipStream_t stream);
// sweep_bwd_det.hip: grad_src of the above as an order-independent sum (fixed_accum.hpp): the same contributions (one kernel body,
// sweep_bwd_body.hpp), quantised per batch item and added as 64-bit integers in the workspace, then converted; the same bits from
// call to call
size_t sweep_backward_det_workspace_bytes(int B, int V, int C, int H, int W);
hipError_t launch_sweep_backward_det(const SweepArgs& a, const float* grad_cost, float* grad_src, void* workspace, hipStream_t stream);

// warp.hip
hipError_t launch_warp_feature(const SweepArgs& a, float* out, hipStream_t stream);
hipError_t launch_sample_coords(const SweepArgs& a, float* ix, float* iy, hipStream_t stream);
// warp_bwd.hip: gradient of launch_warp_feature with respect to src (grad_out, grad_src [B,V,D,H,W] contiguous; a.src is not read):
// float atomics into grad_src, zeroed by the launcher, or -- _det -- an order-independent integer sum in the workspace
hipError_t launch_warp_feature_backward(const SweepArgs& a, const float* grad_out, float* grad_src, hipStream_t stream);
size_t warp_feature_backward_det_workspace_bytes(int B, int V, int D, int H, int W);
hipError_t launch_warp_feature_backward_det(const SweepArgs& a, const float* grad_out, float* grad_src, void* workspace, hipStream_t stream);

// ufield.hip
size_t ufield_workspace_bytes(int B, int H, int W);
hipError_t launch_ufield(const float* dpv, const float* d_candi, const float* intr, const float* mask, int B, int D, int H,
                         int W, int bv_log, float unc_ang, float zstart, float zend, float mind, int quash, float oob_depth,
                         float* plane, float* depth_zero, void* workspace, hipStream_t stream);

// correlation_general.hip (called by the dispatch of correlation.hip): every configuration of the reference's kernel, fp32 or
// fp16 I/O (half != 0), fp32 accumulation
bool correlation_output_size(int H, int W, int pad, int k, int md, int s1, int* oH, int* oW);
hipError_t launch_correlation_general_forward(const void* x1, const void* x2, int half, int B, int C, int H, int W, int pad, int k, int md,
                                              int s1, int s2, void* out, hipStream_t stream);
hipError_t launch_correlation_general_backward(const void* x1, const void* x2, const void* go, int half, int B, int C, int H, int W, int pad,
                                               int k, int md, int s1, int s2, void* g1, void* g2, hipStream_t stream);
// inverse_warp.hip (scatter_det.hip calls it for the gradient of the projected point)
hipError_t launch_inverse_warp_backward(const float* img, const float* depth, const float* Kinv, const float* proj,
                                        const float* grad_out, int B, int C, int H, int W, int mode, float* grad_img,
                                        float* grad_pc, hipStream_t stream);

}  // namespace pdepth
