/*
 * pdepth.h -- C ABI of the MI355X (gfx950) plane-sweep / DPV hot path.
 *
 * Drop-in boundary for soulslicer/probabilistic-depth.  The reference has no FFI on this
 * path: its boundary is a set of Python functions built from ATen ops.  Every entry point
 * below replaces one of them (reference file:line cited per function); the Python host
 * package binds this header with ctypes (probabilistic-depth_amd/_native.py) and
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions (all entry points)
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless a stride argument says
 *     otherwise; strides are in ELEMENTS (floats);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); launches are
 *     asynchronous, no host synchronisation, no allocation -- callers own all buffers
 *     (mirrors the reference's native op: models/correlation_package/correlation_cuda.cc:36-42,76);
 *   - return value 0 = launched, non-zero = PDEPTH_E_* and nothing was launched; the text
 *     is available from pdepth_last_error() (thread local).  Mirrors the reference's
 *     "kernel launcher returns 0/1, wrapper raises" convention
 *     (models/correlation_package/correlation_cuda_kernel.cu:383-392, correlation_cuda.cc:81-83);
 *   - the sweep kernels order their tiles per XCD assuming the SPX partition mode of the MI355X
 *     (workgroup i is dispatched to XCD i mod 8, each XCD with its own L2); under another
 *     partition mode the results are the same and only L2 locality is lost;
 *   - arithmetic: inputs, outputs, sample positions, bilinear weights and every sum are fp32 (SURVEY.md section 8:
 *     d_candi is float64 on the host and cast to fp32 at use, warping/homography.py:115, utils/img_utils.py:58).
 *     ONE step of the default sweep kernel (PDEPTH_ALGO_AUTO / _DIST, L2 metric) is not an fp32 instruction: the channel
 *     contraction <s, r> of the centred features runs on the matrix pipe as products of fp16 high / low PAIRS
 *     (h = fp16(x'), l = fp16(x' - h): 22 bits per feature, products exact, fp32 accumulation;
 *     v_mfma_f32_16x16x32_f16) -- measured as accurate as the fp32 matrix instruction.
 *     BASELINE.json's north star describes the path as "no MFMA (a gather/reduce)": the gather and the reductions are
 *     vector code here too, the contraction over the channels is not (DESIGN.md section 1 says why).  A caller who
 *     wants the reference's own operation order end to end selects PDEPTH_ALGO_DIRECT.
 *   - values that are not numbers propagate as in the reference: a NaN / inf feature or depth candidate makes the costs
 *     it enters, and with them the pixel's log-DPV and depth, non-finite.  A finite feature beyond the fp16 range of the
 *     default kernel's scaled layout (several thousand times the sampled maximum of its batch item): pdepth_sweep_dpv_f32
 *     evaluates that batch item with the gather kernel on the NCHW tensor (right numbers), the packed entry -- which has
 *     no NCHW tensor -- makes the item's outputs NaN: never a clamped number.
 *   - routing (PDEPTH_ALGO_AUTO / _DIST through pdepth_sweep_cost_f32 / pdepth_sweep_dpv_f32): a batch item whose costs are
 *     so large against the candidates' range that two fp32 evaluations agree to 1e-4 m only if they round alike
 *     (V (2 sum_c var_c + |mu|^2) / sigma * (d_max - d_min) * 2^-23 > 4e-4; the headline workload: 5.6e-5), or whose
 *     features carry trends the centring cannot remove, is evaluated by the gather kernel (the reference's operation
 *     order, PDEPTH_ALGO_DIRECT's kernel) inside the same call: ONE more launch, whose blocks leave at once when no item
 *     is flagged.  The packed entry of the default kernel evaluates every item in the distance form (it has no fp32
 *     features to fall back to); the LDS-tiled kernel (L1, C > 72, D > 128, forced selectors) routes on both entries.
 */
#ifndef PDEPTH_H_
#define PDEPTH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDEPTH_ABI_VERSION 6   /* 5: PDEPTH_ALGO_DIST (what AUTO runs), pdepth_sweep_source_layout, layout tag in the workspace;
                                * 6: the distance-form layout is 320 bytes per texel at C = 67 (336 in v5): a workspace packed by a v5
                                *    library must be re-packed; PDEPTH_ALGO_CORR is refused (PDEPTH_E_ARG; since retired with CELLS and MFMA);
                                *    backward-compatible additions within 6: pdepth_sweep_backward_f32, pdepth_dpv_reduce_backward_f32,
                                *    pdepth_dpv_expect_backward_f32; pdepth_dpv_soft_ce_workspace_bytes, pdepth_dpv_soft_ce_f32,
                                *    pdepth_dpv_soft_ce_backward_f32; pdepth_depth_metrics_workspace_bytes, pdepth_depth_metrics_f32;
                                *    pdepth_dpv_fuse_backward_f32; pdepth_lidar_depth_workspace_bytes, pdepth_lidar_depth_f32;
                                *    pdepth_loss_terms_workspace_bytes, pdepth_loss_{dsc,rsc,dc,smooth}_f32 and their _backward_f32;
                                *    PDEPTH_DTYPE_F16 / PDEPTH_DTYPE_BF16, pdepth_dpv_reduce_ex_lp, pdepth_dpv_reduce_backward_lp;
                                *    pdepth_det_scale_exponent and the three _backward_det_f32 entries with their _det_workspace_bytes;
                                *    pdepth_warp_feature_backward_f32, pdepth_warp_feature_backward_det_f32 and its _det_workspace_bytes;
                                *    pdepth_ssim_f32, pdepth_ssim_backward_f32;
                                *    pdepth_loss_photo_workspace_bytes, pdepth_loss_photo_f32, pdepth_loss_photo_backward_f32;
                                *    pdepth_ternary_f32, pdepth_ternary_backward_f32;
                                *    pdepth_range_map_workspace_bytes, pdepth_range_map_f32, pdepth_depth_range_map_f32;
                                *    pdepth_flow_warp_f32, pdepth_flow_warp_backward_f32, pdepth_flow_warp_backward_det_f32 and its
                                *    _det_workspace_bytes, pdepth_flow_fb_check_f32; pdepth_loss_smooth1_f32 and its _backward_f32;
                                *    pdepth_flow_cost_volume_f32, its _backward_f32 and _backward_det_f32 and their workspace queries;
                                *    pdepth_flow_photo_workspace_bytes, pdepth_flow_photo_f32, pdepth_flow_photo_backward_f32;
                                *    pdepth_flow_metrics_workspace_bytes, pdepth_flow_metrics_f32, pdepth_flow_resize_f32 */

enum {
    PDEPTH_OK = 0,
    PDEPTH_E_ARG = 1,       /* bad shape / null pointer / unsupported value      */
    PDEPTH_E_LAUNCH = 2,    /* hipGetLastError() after launch was not success   */
    PDEPTH_E_WORKSPACE = 3  /* workspace too small for the requested algorithm  */
};

/* feature distance, warping/homography.py:128-133 ('L2' | 'L1', anything else raises) */
enum { PDEPTH_METRIC_L2 = 0, PDEPTH_METRIC_L1 = 1 };

/* Rounding of the host BLAS whose sgemm/sgemv the reference's CPU path calls for K@R, K@t and
 * (K@R)@rays (warping/homography.py:119-121).  One ulp of those terms moves the L2 cost by ~1e-3,
 * so "identical to the reference CPU path" depends on which MKL code path the host takes:
 *   FMA      (MKL on Intel AVX-512/AVX2): sgemm = fma chain k=0,1,2 (first product rounded alone);
 *                                         sgemv (K@t) = (p1 + p2) + p0, products rounded separately
 *   SEPARATE (MKL on AMD EPYC)          : sgemm and sgemv = (p0 + p1) + p2, products rounded separately
 * The Python host probes torch's CPU matmul once and passes the matching mode
 * (probabilistic-depth_amd/_native.py host_blas_mode()). */
enum { PDEPTH_BLAS_FMA = 0, PDEPTH_BLAS_SEPARATE = 1 };

/* algorithm selector for the sweep kernels (pdepth_sample_coords_f32 reports the positions of the same
 * selector: AUTO = explicit shared-reciprocal fma divide chain, DIRECT = compiler IEEE divides; the two are
 * bit-identical for every position within reach of the image, tests/test_hip_parity.py) */
enum {
    PDEPTH_ALGO_AUTO = 0,    /* fastest algorithm valid for the given geometry          */
    PDEPTH_ALGO_DIRECT = 1,  /* per-plane bilinear gather, reference op order (any pose) */
    /* implementation selectors (parity tests, A/B timing): what AUTO may pick, forced.  Same workspace as AUTO. */
    PDEPTH_ALGO_TILED_1 = 2, /* LDS-tiled band kernel, one 16x4 tile per block                          */
    PDEPTH_ALGO_TILED_2 = 3, /* LDS-tiled band kernel, two tiles per block (D <= 64)                    */
    /* retired values: the numbers stay reserved, a descriptor that names one is refused with PDEPTH_E_ARG */
    PDEPTH_ALGO_CELLS = 4,   /* RETIRED: cell-list kernels of round 2                                               */
    PDEPTH_ALGO_MFMA = 5,    /* RETIRED: fp32 matrix-pipe kernel of round 3                                         */
    PDEPTH_ALGO_CORR = 6,    /* RETIRED: correlation form on mean-centred features (the default of ABI 4)           */
    PDEPTH_ALGO_DIST = 7     /* distance form sum_t w_t |s_t - r|^2 - Q on fp16 high / low parts, matrix pipe (L2 metric,
                                D <= 128, C <= 72, V <= 8; other inputs: PDEPTH_E_ARG): what AUTO runs on those shapes  */
};

/* staging layouts of the packed source (pdepth_sweep_source_layout) */
enum {
    PDEPTH_LAYOUT_NONE = 0,        /* the descriptor does not run on a packed source                                   */
    PDEPTH_LAYOUT_C4 = 1,          /* channel-group-planar float4 + Gram planes (LDS-tiled kernel)                     */
    PDEPTH_LAYOUT_C4_CENTRED = 2,  /* RETIRED (was PDEPTH_ALGO_CORR's): the number stays reserved, no descriptor selects it */
    PDEPTH_LAYOUT_DIST16 = 3       /* fp16 high / low planes in matrix-operand order + neighbour differences, ring of
                                      zero-feature texels (PDEPTH_ALGO_DIST; csrc/dist_layout.hpp)                     */
};

/* Geometry + layout of one batched sweep call. */
typedef struct pdepth_sweep_desc {
    int32_t B;           /* batch items (depth volumes)                                 */
    int32_t V;           /* source views per item (reference view excluded)             */
    int32_t C;           /* feature channels (67 = 64 learned + 3 rgb, models.py:518-520)*/
    int32_t D;           /* depth planes                                                */
    int32_t H, W;        /* sweep resolution                                            */
    int32_t metric;      /* PDEPTH_METRIC_*                                             */
    int32_t algo;        /* PDEPTH_ALGO_*                                               */
    int32_t blas_mode;   /* PDEPTH_BLAS_* : rounding of K@R, K@t, (K@R)@rays            */
    float sigma;         /* costV_sigma (cfg.var.sigma_soft_max, 10.0)                  */
    int64_t ref_bstride; /* elements between ref[b] and ref[b+1]   (>= C*H*W)           */
    int64_t src_bstride; /* elements between src[b,0] and src[b+1,0]                    */
    int64_t src_vstride; /* elements between src[b,v] and src[b,v+1] (>= C*H*W)         */
} pdepth_sweep_desc;

/* Camera of one batched sweep call (all device pointers). */
typedef struct pdepth_camera {
    const float *K;     /* [B,3,3]   intrinsic_M_cuda             (models.py:537)        */
    const float *R;     /* [B,V,3,3] src_cam_poses[b,v,:3,:3]     (models.py:530)        */
    const float *t;     /* [B,V,3]   src_cam_poses[b,v,:3,3]      (models.py:531)        */
    const float *rays;  /* [B,3,H*W] unit_ray_array_2D, col=y*W+x (models.py:539)        */
    const float *cxcy;  /* [B,2]     float32(intrinsic_M[0,2]), float32(intrinsic_M[1,2])
                                     (warping/homography.py:194)                         */
} pdepth_camera;

int pdepth_abi_version(void);
const char *pdepth_last_error(void);

/*
 * Plane-sweep cost volume.  Replaces est_swp_volume_v4 (warping/homography.py:98-135) +
 * _back_warp_homo_parallel (:170-198) + img_dis_L2_pard/img_dis_L1_pard (:80-86), batched
 * over the Python loop at models/models.py:528-550.
 *   ref  [B,C,H,W] (ref_bstride), src [B,V,C,H,W] (src_bstride/src_vstride), d_candi [D]
 *   cost [B,D,H,W] contiguous, fully overwritten:
 *   cost[b,k,y,x] = sum_v ( sum_c dist(warp_{v,k}(src)[c,y,x], ref[c,y,x]) / sigma )
 */
int pdepth_sweep_cost_f32(const pdepth_sweep_desc *desc, const pdepth_camera *cam,
                          const float *ref, const float *src, const float *d_candi,
                          float *cost, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Fused sweep + DPV reduction: cost -> log_softmax over D -> E[d].  Replaces the chain
 * est_swp_volume_v4 -> F.log_softmax(dim=1) (models/packnet.py:380-394) ->
 * dpv_to_depthmap(BV_log=True) (utils/img_utils.py:52-61) without writing the cost volume.
 *   cost  [B,D,H,W] or NULL     (un-normalised cost, as pdepth_sweep_cost_f32)
 *   logp  [B,D,H,W] or NULL     (log DPV)
 *   depth [B,H,W]   or NULL     (expected depth)
 * At least one output must be non-NULL.
 */
int pdepth_sweep_dpv_f32(const pdepth_sweep_desc *desc, const pdepth_camera *cam,
                         const float *ref, const float *src, const float *d_candi,
                         float *cost, float *logp, float *depth,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same fused sweep for a caller that keeps its source features in the kernels' staging layout -- e.g. the epilogue
 * of the feature encoder (models/models.py:518-534 is where the reference concatenates the 64 learned channels with
 * the RGB thumbnail) -- so that the re-layout is paid once per frame instead of once per sweep call (it is a fifth of the
 * time of pdepth_sweep_dpv_f32 on the headline shape):
 *   pdepth_pack_source_f32      : src [B,V,C,H,W] (strides from desc) -> workspace, in the layout the sweep kernel that
 *                                 `desc` selects reads (pdepth_sweep_source_layout(desc)):
 *                                   PDEPTH_LAYOUT_DIST16 (L2, C <= 72, D <= 128, V <= 8: what AUTO runs): per view an
 *                                     (H + 2) x wp(W) image (a ring of zero-feature texels; rows padded to a multiple of 8
 *                                     texels), planes of 16 bytes per texel: the centred, power-of-two scaled features as
 *                                     fp16 high and low parts in matrix-operand order, |x'|^2 as three fp16 pieces, and an
 *                                     fp32 record of the five squared neighbour differences of the cell (20 planes = 320
 *                                     bytes per texel at C = 67), stored texel-group-major: the planes of four consecutive
 *                                     texels of a row lie together (1 280 bytes at C = 67; csrc/dist_layout.hpp);
 *                                   PDEPTH_LAYOUT_C4 (L1 metric, C > 72, D > 128: the LDS-tiled kernel): float4 texels of 4
 *                                     channels, planes [ceil(C/4)][H][W], + 2 Gram planes;
 *   pdepth_sweep_dpv_packed_f32 : the sweep on a workspace packed by that call for a desc with the same B, V, C, H, W and
 *                                 the SAME pdepth_sweep_source_layout() -- a layout is tied to its kernel family: the
 *                                 metric and the algo selector may only change within it (any cameras, depth candidates,
 *                                 sigma, reference features).  Outputs as pdepth_sweep_dpv_f32.  A foreign layout is
 *                                 detected on the device (tag in the workspace): every output is filled with NaN.
 *                                 The packed entry of the default kernel is ONE launch.
 * PDEPTH_E_ARG if the shape does not run on a packed source (then use pdepth_sweep_dpv_f32).
 * Statistics.  The default kernel centres and scales with per-channel constants of the batch item, estimated from sampled
 * rows: pdepth_sweep_dpv_f32 and pdepth_pack_views_f32 sample every source view AND the reference view,
 * pdepth_pack_source_f32 (which is not given the reference) the source views.
 */
int pdepth_pack_source_f32(const pdepth_sweep_desc *desc, const float *src, void *workspace,
                           size_t workspace_bytes, void *stream);
/*
 * The encoder epilogue, fused with that re-layout: replaces
 *     feat_imgs_all = torch.cat((feat_imgs, F.avg_pool2d(rgb, dw_rate)), dim=1)     models/models.py:518-520, packnet.py:355-357
 *     feat_img_ref = feat_imgs_all[i, -1], feat_imgs_src = feat_imgs_all[i, :-1]    models/models.py:530-534
 * and pdepth_pack_source_f32 with ONE pass over the encoder output:
 *   feat [B*(V+1), C-3, H, W] (the encoder's feature maps, view V of every item = the reference view),
 *   rgb  [B*(V+1), 3, H*pool_rate, W*pool_rate] (the frames; pooled like F.avg_pool2d(kernel = stride = pool_rate)),
 *   -> workspace: the V source views of every item in the staging layout (for pdepth_sweep_dpv_packed_f32, same desc),
 *   -> ref_out [B, C, H, W]: the reference view's features, NCHW (what that entry takes as `ref`).
 * desc: B, V (source views), C (= encoder channels + 3), D, H, W, algo = PDEPTH_ALGO_AUTO.
 */
int pdepth_pack_views_f32(const pdepth_sweep_desc *desc, const float *feat, const float *rgb, int32_t pool_rate,
                          float *ref_out, void *workspace, size_t workspace_bytes, void *stream);
int pdepth_sweep_dpv_packed_f32(const pdepth_sweep_desc *desc, const pdepth_camera *cam, const float *ref,
                                const float *d_candi, float *cost, float *logp, float *depth,
                                void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of scratch the two sweep entry points need for `desc` (0 for ALGO_DIRECT); the workspace
 * must be 256-byte aligned.  ALGO_AUTO without it returns PDEPTH_E_WORKSPACE.  It holds two ints per 16x4 tile (tile flags
 * and the list of left-over tiles of the LDS-tiled kernel; the default kernel keeps its eight per-XCD queue counters in the
 * first, 256 bytes apart), 64 counter / tag ints, the packed source views -- sized for the LARGEST of the layouts of the shape, so any pack fits any sweep:
 * max(B*V*(8*nchk(C)+4)*(H+2)*wp(W)*16 + 256*B*V, B*V*(ceil(C/4)+2)*H*W*16) bytes with nchk(C) = 0 | 1 | 2 chunks of 32
 * channels and wp(W) = W + 2 rounded up to a multiple of 8 -- and 496 floats of channel statistics per batch item.  Size it
 * once per shape and reuse it.  A call rewrites all of it: do not share one workspace between calls that may run
 * concurrently (different streams). */
size_t pdepth_sweep_workspace_bytes(const pdepth_sweep_desc *desc);

/* 1 if the packing entry points (pdepth_pack_source_f32, pdepth_pack_views_f32) subtract the channel means from the
 * packed source for `desc` -- i.e. the sweep it selects is the distance-form kernel (PDEPTH_ALGO_DIST, directly or through
 * PDEPTH_ALGO_AUTO) --, else 0.  A packed workspace must be swept with a descriptor for which this answer is the same (the centred and the
 * plain layout differ; the library cannot tell them apart from the host).  No reference counterpart: the reference
 * never re-lays its features (warping/homography.py:123-129 works on the NCHW tensors). */
int pdepth_sweep_centres_source(const pdepth_sweep_desc *desc);

/* Which staging layout (PDEPTH_LAYOUT_*) the packing entry points write for `desc`, i.e. which kernel family the sweep it
 * selects belongs to.  A packed workspace must be swept with a descriptor for which this answer is the same.  The pack
 * kernels also write the answer into the workspace, and a sweep kernel that finds another family's tag there fills its
 * outputs with NaN instead of returning numbers computed from the wrong bytes.  No reference counterpart (as above). */
int pdepth_sweep_source_layout(const pdepth_sweep_desc *desc);

/*
 * DPV reduction: logits [B,D,H,W] -> logp [B,D,H,W] (may alias logits, may be NULL) and
 * depth [B,H,W] (may be NULL).  Replaces F.log_softmax(x, dim=1) (models/models.py:560,637,
 * 694, :351) followed by dpv_to_depthmap(., BV_log=True) (utils/img_utils.py:52-61;
 * trainer/default_trainer.py:229-233) in one pass over the logits.
 */
int pdepth_dpv_reduce_f32(const float *logits, const float *d_candi, int32_t B, int32_t D,
                          int32_t H, int32_t W, float *logp, float *depth, void *stream);

/*
 * The same single pass with optional extras (any output may be NULL, not all): replaces, next to the lines above,
 *   addend       [B,D,H,W] or NULL : x = logits + addend before the softmax -- the feedback update
 *                                    F.log_softmax(BV_cur + BV_resi, dim=1)            (models/models.py:694)
 *   prob         [B,D,H,W]         : exp(logp), the decoder's input torch.exp(BV_cur_upd) (models/models.py:697, :651)
 *   variance     [B,H,W]           : sum_k (d_k - E[d])^2 p_k, the inline lines of the evaluation loop
 *                                                                        (trainer/default_trainer.py:333-336)
 *   logp_quarter [B,D,H/4,W/4]     : F.interpolate(logp, scale_factor=0.25, mode='nearest'), the prev_output of the
 *                                    next frame                          (trainer/default_trainer.py:221)
 * logp may alias logits; no other aliasing.
 */
int pdepth_dpv_reduce_ex_f32(const float *logits, const float *addend, const float *d_candi, int32_t B, int32_t D,
                             int32_t H, int32_t W, float *logp, float *prob, float *depth, float *variance,
                             float *logp_quarter, void *stream);

/* the 2-byte element types of the _lp entries (0 and every other value: PDEPTH_E_ARG) */
enum { PDEPTH_DTYPE_F16 = 1, PDEPTH_DTYPE_BF16 = 2 };

/*
 * pdepth_dpv_reduce_ex_f32 on half-precision logits, as a model under torch.autocast hands them over: logits and the
 * optional addend [B,D,H,W] are IEEE binary16 (PDEPTH_DTYPE_F16) or bfloat16 (PDEPTH_DTYPE_BF16), both of the one dtype.
 * Every element is widened to fp32 where it is loaded, which is exact, and nothing else changes: every sum is the fp32 one
 * of pdepth_dpv_reduce_ex_f32, in its order, so logp, depth, variance and logp_quarter (fp32, shapes and the H, W >= 4 rule
 * as there) have the bits pdepth_dpv_reduce_ex_f32 gives on the widened input.  prob is fp32 (prob_is_lp = 0) or of the
 * logits' dtype (prob_is_lp != 0): the fp32 value rounded to nearest-even where it is stored.  The cast costs no pass of its
 * own: 6 bytes per element for logp against 14 for a cast followed by the fp32 entry.
 * logp is fp32 and so cannot alias the half-precision logits; no output may alias an input.  A volume whose base address
 * is not 8-byte aligned (a 2-byte view may start 2 bytes into its storage), W % 4 != 0 or D > 128 runs one pixel per thread.
 */
int pdepth_dpv_reduce_ex_lp(int32_t dtype, const void *logits, const void *addend, const float *d_candi, int32_t B, int32_t D,
                            int32_t H, int32_t W, float *logp, void *prob, int32_t prob_is_lp, float *depth, float *variance,
                            float *logp_quarter, void *stream);

/*
 * Expectation only: depth[b,y,x] = sum_k d_k * (bv_log ? exp(dpv[b,k,y,x]) : dpv[b,k,y,x]).
 * Replaces dpv_to_depthmap (utils/img_utils.py:52-61), batched over B.
 */
int pdepth_dpv_expect_f32(const float *dpv, const float *d_candi, int32_t B, int32_t D,
                          int32_t H, int32_t W, int32_t bv_log, float *depth, void *stream);

/*
 * Mean and variance of the depth distribution: z = bv_log ? exp(dpv) : dpv, mean = sum_k d_k z_k,
 * variance[b,y,x] = sum_k (d_k - mean)^2 z_k.  Replaces the per-item torch ops of the evaluation loop
 * (trainer/default_trainer.py:333-336), batched over B.  mean may be NULL.
 */
int pdepth_dpv_moments_f32(const float *dpv, const float *d_candi, int32_t B, int32_t D,
                           int32_t H, int32_t W, int32_t bv_log, float *mean, float *variance, void *stream);

/*
 * Diagonal feature warp: out[b,v,i,y,x] = bilinear(src[b,v,i,:,:]) sampled with the
 * plane-i homography of view v.  Replaces warp_feature (warping/homography.py:137-168),
 * which warps all D x C planes and keeps [i,i]; requires C == D.
 *   desc->C must equal desc->D; desc->V counts ALL views passed (reference view included,
 *   models/models.py:616-617); src [B,V,D,H,W] via src_bstride/src_vstride; out contiguous.
 */
int pdepth_warp_feature_f32(const pdepth_sweep_desc *desc, const pdepth_camera *cam,
                            const float *src, const float *d_candi, float *out, void *stream);

/*
 * Sampling coordinates only (diagnostic, used by the parity tests to pin the coordinate
 * pipeline bit-for-bit): ix, iy [B,V,D,H,W] = un-normalised pixel coordinates handed to the
 * bilinear sampler (warping/homography.py:185-196 + ATen grid_sampler unnormalize).
 */
int pdepth_sample_coords_f32(const pdepth_sweep_desc *desc, const pdepth_camera *cam,
                             const float *d_candi, float *ix, float *iy, void *stream);

/*
 * Uncertainty-field collapse: replaces gen_ufield (utils/img_utils.py:268-358; called through compute_unc_field
 * :178-181 by the evaluation loop, trainer/default_trainer.py:243-244), batched over B.
 *   dpv [B,D,H,W] (log-DPV if bv_log, else probabilities), intr [B,3,3] full-resolution intrinsics, mask [B,H,W] or
 *   NULL (validity of the ground-truth volume).  unc_ang = rows the volume is shifted by (cfgx["unc_ang"]; 0 = no
 *   shift; a shift needs H, W >= 2, its sampling grid divides by size - 1), [z_start, z_end] = height band (cfgx: unc_shift, unc_shift + unc_span), min_depth / quash as in the
 *   reference's branches (:269-290: cfgx and ILIM 3 / 1, KITTI 0 / 0), oob_depth = the depth the reference assigns to
 *   rows shifted in from outside (sum_k d_k for a log-DPV -- exp of the zero padding -- else 0).
 *   plane [B,D,W] = per column the mean depth distribution of the pixels in the band (NaN for columns without one, as
 *   in the reference), depth_zero [B,H,W] = E[d] masked to those pixels.  The min/max normalisation (:353-355) is a
 *   [D,W] post-process left to the host.  Workspace: pdepth_ufield_workspace_bytes (two [B,H,W] maps + [B,W]).
 */
size_t pdepth_ufield_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pdepth_ufield_f32(const float *dpv, const float *d_candi, const float *intr, const float *mask, int32_t B,
                      int32_t D, int32_t H, int32_t W, int32_t bv_log, float unc_ang, float z_start, float z_end,
                      float min_depth, int32_t quash, float oob_depth, float *plane, float *depth_zero,
                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * DPV Bayesian fusion of the upsample mode: replaces gen_dpv_withmask (utils/img_utils.py:360-375, with
 * gen_soft_label_torch :31-47 and gen_uniform :49-50) followed by the fuse / renormalise / clamp / log
 * lines of BaseModel.forward_int (models/models.py:666-672).
 *   logp [B,D,H,W] log-DPV of the network, dmaps [B,H,W] sparse depth, masks [B,H,W] validity (channel 0
 *   of the reference's [B,1,H,W]), var = 0.3 in the reference, eps = torch.finfo(float).eps.
 *   fused [B,D,H,W] (clamped probabilities) and logfused [B,D,H,W]; either may be NULL, not both.  H*W <= 2^30, B <= 65535.
 *   A column of logp with a NaN, with -inf on every plane or whose exp overflows comes out as eps (log eps) on every plane,
 *   where the reference returns NaN; the backward returns non-finite values on such a column.
 */
int pdepth_dpv_fuse_f32(const float *logp, const float *dmaps, const float *masks, const float *d_candi,
                        int32_t B, int32_t D, int32_t H, int32_t W, float var, float eps, float *fused,
                        float *logfused, void *stream);

/*
 * Backward of pdepth_dpv_fuse_f32 with respect to logp (what autograd does behind models/models.py:666-672 for BV_cur; the
 * prior of gen_dpv_withmask, utils/img_utils.py:360-375, is built from data and is constant).  Per pixel, with m the clamped
 * prior the forward builds:
 *     u = exp(logp + log m),  q = u / sum_k u_k             (fused = clamp(q, eps, 1), logfused = log fused)
 *     c = pass (g_fused q + g_logfused),  pass = (eps <= q <= 1), torch.clamp's rule
 *     g_logp = c - q sum_k c_k
 *   logp, dmaps, masks, d_candi, B, D, H, W, var, eps as in the forward: m and q are recomputed from them with the forward's
 *   arithmetic, neither output volume is needed;
 *   g_fused, g_logfused [B,D,H,W] contiguous, either may be NULL (= zero, and not read), not both;
 *   g_logp [B,D,H,W], may not alias an input.  No atomics: reproducible bit for bit.  H*W <= 2^30, B <= 65535.
 */
int pdepth_dpv_fuse_backward_f32(const float *logp, const float *dmaps, const float *masks, const float *d_candi,
                                 const float *g_fused, const float *g_logfused, int32_t B, int32_t D, int32_t H, int32_t W,
                                 float var, float eps, float *g_logp, void *stream);

/*
 * The reference's native correlation operator, forward and backward: replaces correlation_forward_cuda /
 * correlation_backward_cuda (models/correlation_package/correlation_cuda.cc:10-87, :89-167; kernels
 * correlation_cuda_kernel.cu:41-114, :116-300) with the reference's argument list (the rbot1 / rbot2 scratch tensors --
 * zero-padded NHWC repacks -- are not needed).  Every configuration the reference's kernel defines:
 *     kr = (kernel_size-1)/2, dr = max_displacement/stride2, ds = 2 dr + 1
 *     output [B, ds*ds, oH, oW], oH = ceil((H + 2 pad_size - 2 (kr + max_displacement)) / stride1) (correlation_cuda.cc:24-33;
 *     pdepth_correlation_output_size), channel (tj+dr)*ds + (ti+dr),
 *     out = 1/(k*k*C) sum_{j,i in [-kr,kr]} sum_c in1p[y1+j, x1+i] * in2p[y1 + tj*stride2 + j, x1 + ti*stride2 + i],
 *     (y1, x1) = (oy, ox) * stride1 + max_displacement in the coordinates of the zero-padded inputs.
 * kernel_size must be odd and (kernel_size-1)/2 <= max_displacement mod stride2 (beyond that the reference's kernel reads
 * outside its padded buffers); corr_multiply is accepted and ignored like in the reference kernel.  The configuration the
 * reference instantiates (kernel 1, stride1 1, pad_size = max_displacement <= 4*stride2: pwclite.py:123-125) runs
 * tiled fp32 kernels as far as their tile fits the 160 KiB of LDS (forward: max_displacement <= 144; backward:
 * max_displacement <= 17); beyond that, everything else, and the fp16 entries (fp16 tensors, fp32 accumulation:
 * AT_DISPATCH_FLOATING_TYPES_AND_HALF at correlation_cuda_kernel.cu:352-369), a general gather kernel: which kernel serves
 * a call is decided before anything is launched, and no accepted configuration is refused for its size of tile.
 * Non-finite values: the zeros of the padding are multiplied, not skipped, as in the reference's padded buffers
 * (correlation_cuda_kernel.cu:88-96): an inf or NaN of one input paired with padding of the other (or, in the backward, an
 * inf or NaN of grad_output paired with padding) gives NaN, on every kernel and in both types alike.
 *   forward : input1, input2 [B,C,H,W] -> output;   backward: grad_output [B,ds*ds,oH,oW] -> grad_input1, grad_input2
 *   [B,C,H,W] (either may be NULL).
 */
int pdepth_correlation_output_size(int32_t H, int32_t W, int32_t pad_size, int32_t kernel_size, int32_t max_displacement,
                                   int32_t stride1, int32_t stride2, int32_t *out_channels, int32_t *out_height,
                                   int32_t *out_width);
int pdepth_correlation_forward_f32(const float *input1, const float *input2, int32_t B, int32_t C, int32_t H,
                                   int32_t W, int32_t pad_size, int32_t kernel_size, int32_t max_displacement,
                                   int32_t stride1, int32_t stride2, int32_t corr_multiply, float *output,
                                   void *stream);
int pdepth_correlation_backward_f32(const float *input1, const float *input2, const float *grad_output, int32_t B,
                                    int32_t C, int32_t H, int32_t W, int32_t pad_size, int32_t kernel_size,
                                    int32_t max_displacement, int32_t stride1, int32_t stride2,
                                    int32_t corr_multiply, float *grad_input1, float *grad_input2, void *stream);
int pdepth_correlation_forward_f16(const void *input1, const void *input2, int32_t B, int32_t C, int32_t H, int32_t W,
                                   int32_t pad_size, int32_t kernel_size, int32_t max_displacement, int32_t stride1,
                                   int32_t stride2, int32_t corr_multiply, void *output, void *stream);
int pdepth_correlation_backward_f16(const void *input1, const void *input2, const void *grad_output, int32_t B,
                                    int32_t C, int32_t H, int32_t W, int32_t pad_size, int32_t kernel_size,
                                    int32_t max_displacement, int32_t stride1, int32_t stride2, int32_t corr_multiply,
                                    void *grad_input1, void *grad_input2, void *stream);

/*
 * Depth-map driven inverse warp: replaces the per-pixel part of inverse_warp (utils/inverse_warp.py:174-210 with
 * pixel2cam :26-40 and cam2pixel :43-69), used by the training losses (losses/loss_blocks.py:116 with the default
 * 'bilinear', :151 with 'nearest').  The host supplies Kinv = intrinsics.inverse() [B,3,3] and
 * proj = intrinsics @ pose_mat [B,3,4] (:193-203); img [B,C,H,W], depth [B,H,W] ->
 * out [B,C,H,W] (zeros padding, grid_sample's default align_corners=False) and valid [B,H,W] as bytes
 * (|normalised coordinate| <= 1, :208), valid may be NULL.
 */
enum { PDEPTH_SAMPLE_BILINEAR = 0, PDEPTH_SAMPLE_NEAREST = 1 };
int pdepth_inverse_warp_f32(const float *img, const float *depth, const float *Kinv, const float *proj,
                            int32_t B, int32_t C, int32_t H, int32_t W, int32_t mode, float *out, uint8_t *valid,
                            void *stream);

/*
 * Backward of the same (what autograd does behind the reference's call, through F.grid_sample and the projection):
 *   grad_out [B,C,H,W] -> grad_img [B,C,H,W] (fully overwritten: cleared, then scattered with atomics like ATen's
 *   grid_sampler backward; may be NULL) and grad_point [B,3,H,W] = dL/d(X, Y, Z) of the projected point
 *   proj[:, :, :3] @ cam + proj[:, :, 3] of every pixel (may be NULL; zero in nearest mode).  The gradients of the
 *   depth map, the pose and the intrinsics follow from grad_point by the 3x3 / 3x4 products the host already owns
 *   (probabilistic-depth_amd/utils/inverse_warp.py does them in torch).
 */
int pdepth_inverse_warp_backward_f32(const float *img, const float *depth, const float *Kinv, const float *proj,
                                     const float *grad_out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t mode,
                                     float *grad_img, float *grad_point, void *stream);

/*
 * Backward of the plane sweep with respect to the feature maps (what autograd does behind est_swp_volume_v4,
 * warping/homography.py:98-135: F.grid_sample bilinear / zeros / align_corners=False at :170-198, img_dis_L2_pard /
 * img_dis_L1_pard at :80-86, the division by sigma at :131-134; trained through losses/losses.py:80-88).
 *   desc, cam, ref, src, d_candi as pdepth_sweep_cost_f32 (desc->metric selects L2 / L1; desc->algo is ignored: the
 *   backward evaluates every plane directly in fp32 on the NCHW features, positions from the gather kernel's arithmetic);
 *   grad_cost [B,D,H,W] contiguous;
 *   grad_ref  [B,C,H,W] contiguous or NULL: a per-pixel gather, no atomics, bitwise reproducible;
 *   grad_src  [B,V,C,H,W] contiguous or NULL: zeroed on the stream by a launch (not a memset: the call can be captured and
 *             replayed), then scattered with float atomics (summed per workgroup in LDS first); the last bits depend on the order in which the adds arrive (pdepth_sweep_backward_det_f32: they do not).
 * At least one output must be non-NULL.  Taps outside the image receive nothing (ATen's grid_sampler_2d backward).
 */
int pdepth_sweep_backward_f32(const pdepth_sweep_desc *desc, const pdepth_camera *cam, const float *ref, const float *src,
                              const float *d_candi, const float *grad_cost, float *grad_ref, float *grad_src, void *stream);

/*
 * Backward of pdepth_dpv_reduce_f32 / pdepth_dpv_reduce_ex_f32 (F.log_softmax(dim=1), models/models.py:560,637,694; exp,
 * :697; dpv_to_depthmap(BV_log=True), utils/img_utils.py:52-61): from the saved logp [B,D,H,W] and any of
 * g_logp [B,D,H,W], g_prob [B,D,H,W], g_depth [B,H,W] (NULL = zero; not all NULL):
 *     G = g_logp + p (g_prob + g_depth d),  g_logits = G - p sum_k G_k,  p = exp(logp).
 * g_logits [B,D,H,W] is also the gradient of the addend of pdepth_dpv_reduce_ex_f32.  g_logits may alias g_logp.
 */
int pdepth_dpv_reduce_backward_f32(const float *logp, const float *d_candi, int32_t B, int32_t D, int32_t H, int32_t W,
                                   const float *g_logp, const float *g_prob, const float *g_depth, float *g_logits,
                                   void *stream);

/*
 * Backward of pdepth_dpv_reduce_ex_lp: pdepth_dpv_reduce_backward_f32 with g_logits [B,D,H,W] stored in `dtype`, the fp32
 * value rounded to nearest-even, and g_prob read in fp32 (g_prob_is_lp = 0) or in `dtype` (g_prob_is_lp != 0: the type prob
 * was emitted in), widened where it is loaded.  logp, g_logp and g_depth are fp32, and so is every sum: one thread per pixel,
 * planes ascending, the bits of pdepth_dpv_reduce_backward_f32 rounded once.  g_logits may alias no input.
 */
int pdepth_dpv_reduce_backward_lp(int32_t dtype, const float *logp, const float *d_candi, int32_t B, int32_t D, int32_t H,
                                  int32_t W, const float *g_logp, const void *g_prob, int32_t g_prob_is_lp,
                                  const float *g_depth, void *g_logits, void *stream);

/*
 * Backward of pdepth_dpv_expect_f32 (dpv_to_depthmap, utils/img_utils.py:52-61):
 *     g_dpv[b,k,y,x] = g_depth[b,y,x] d_k (bv_log ? exp(dpv[b,k,y,x]) : 1).
 */
int pdepth_dpv_expect_backward_f32(const float *dpv, const float *d_candi, int32_t B, int32_t D, int32_t H, int32_t W,
                                   int32_t bv_log, const float *g_depth, float *g_dpv, void *stream);

/*
 * Training loss on a log-DPV: soft-label cross-entropy over the depth axis, fused with the expectation, for the whole batch in
 * one call (soft_cross_entropy_loss(BV_log=True), losses/loss_blocks.py:186-202, called per item and per side at
 * losses/losses.py:32-67; dpv_to_depthmap(BV_log=True), utils/img_utils.py:52-61, called again at losses/losses.py:80-88).
 *   logp     [B,D,H,W] contiguous fp32 log-probabilities; d_candi [D];
 *   label    [B,D,H,W] contiguous soft label (the loader's soft_labels / soft_labels_imgsize), or NULL;
 *   depth_gt [B,H,W] depth map, or NULL: the label is formed in the kernel as gen_soft_label_torch(d_candi, depth_gt, variance,
 *            zero_invalid=True, pow) does (utils/img_utils.py:24-47; kittiloader/batch_scheduler.py:99-109):
 *            g_d = exp(-|d_d - depth|^pow / (2 sqrt(variance)^pow)), label_d = g_d / sum_d g_d, and -1 on every plane of a pixel
 *            whose sum is 0 or NaN.  No label tensor is read or written.  variance > 0, pow > 0 (2 in the reference);
 *            exactly one of label / depth_gt is non-NULL;
 *   mask     [B,H,W] or NULL.
 *     ce[b,p]   = - sum_d label[b,d,p] logp[b,d,p]
 *     loss[b]   = sum_p ce[b,p] mask[b,p] / count[b],   count[b] = #{p : mask[b,p] == 1}   (the weight is the mask's value, the
 *                 count the number of entries equal to one, as in the reference); 0 where count[b] == 0; pixels whose mask is 0
 *                 are skipped, not multiplied; without a mask the mean over all pixels, count[b] = H W
 *     depth[b,p]= sum_d d_d exp(logp[b,d,p])   (depth NULL = not wanted): the bits of pdepth_dpv_expect_f32(bv_log = 1)
 *   loss [B], count [B] (float).  The volume is read once.  The sum over pixels is reproducible bit for bit: one partial sum per
 *   workgroup of 256 pixels in the workspace, added in a fixed order by a second launch -- no atomics.
 *   workspace: pdepth_dpv_soft_ce_workspace_bytes(B, H, W) bytes (8 bytes per 256 pixels), 256-byte aligned.
 */
size_t pdepth_dpv_soft_ce_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pdepth_dpv_soft_ce_f32(const float *logp, const float *d_candi, const float *label, const float *depth_gt, float variance,
                           float pow, const float *mask, int32_t B, int32_t D, int32_t H, int32_t W, float *loss, float *count,
                           float *depth, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward of pdepth_dpv_soft_ce_f32 with respect to logp (what autograd does behind losses/loss_blocks.py:186-202 and
 * utils/img_utils.py:52-61), one pass, one store per element:
 *     g_logp[b,d,p] = - g_loss[b] mask[b,p] / count[b] label[b,d,p]        (0 where count[b] == 0 or mask[b,p] == 0)
 *                   + g_depth[b,p] d_d exp(logp[b,d,p])                     (g_depth [B,H,W] or NULL = zero)
 *   label / depth_gt / variance / pow / mask as in the forward (the label is formed again from depth_gt), count [B] from the
 *   forward, g_loss [B] or NULL = zero (not both NULL).  The label, the mask, depth_gt and d_candi are data: no gradient.
 */
int pdepth_dpv_soft_ce_backward_f32(const float *logp, const float *d_candi, const float *label, const float *depth_gt,
                                    float variance, float pow, const float *mask, const float *count, int32_t B, int32_t D,
                                    int32_t H, int32_t W, const float *g_loss, const float *g_depth, float *g_logp, void *stream);

/*
 * Evaluation metrics: the KITTI devkit's nine depth errors per item of a batch, on the device (the tail of the evaluation loop,
 * trainer/default_trainer.py:247-256, composed with img_utils.depth_error, utils/img_utils.py:17-22, and depthError,
 * external/deval_lib/src/evaluate_depth.h:20-121; no copy of a depth map to the host).
 *   Exactly one of the two predictions is non-NULL:
 *   pred     [B,H,W] depth maps (any shape), or
 *   logp     [B,D,H,W] contiguous fp32 log-probabilities with d_candi [D]: the prediction is the expectation
 *            sum_d d_d exp(logp[b,d,y,x]), formed in registers from one read of the volume, the bits of
 *            pdepth_dpv_expect_f32(bv_log = 1); depth [B,H,W] (or NULL = not wanted; volume form only) receives it from the same pass;
 *   truth    [B,H,W];  mask [B,H,W] or NULL;  clamp_max <= 0: no clamp (the trainer passes the last depth candidate).
 *     p = pred[b,y,x] mask[b,y,x]                          (no mask: p = pred)
 *     t = truth[b,y,x];  t = clamp_max where t >= clamp_max;  t = -1 where t == 0
 *     valid <=> p > 0                                       (p == 0 is invalid, a NaN is invalid); n = number of valid pixels
 *     e = |p - t|, ei = |1/p - 1/t|, s = log p - log t, el = |s|, sums over the valid pixels:
 *     metrics[b] = { mae = S e / n, rmse = sqrt(S e^2 / n), inverse mae = S ei / n, inverse rmse = sqrt(S ei^2 / n),
 *                    log mae = S el / n, log rmse = sqrt(S el^2 / n), scale invariant log = sqrt(S el^2 / n - (S s)^2 / n^2),
 *                    abs relative = S (e / p) / n, squared relative = S (e^2 / p^2) / n }
 *   The reference's argument order is kept: depth_error(predicted, truth) hands its arguments to depthError(D_gt, D_ipol) in
 *   that order, so validity is decided by the masked prediction and the two relative errors have the prediction as denominator
 *   (not the ground truth).  A valid pixel whose truth is 0 or negative makes the log and inverse metrics of its item NaN, as in
 *   the reference.  Where the reference throws (n == 0) the nine values of that item are NaN and count[b] = 0.
 *   metrics [B,9], count [B] (float, = n).  The per-pixel terms are fp32, their sums fp64; reproducible bit for bit: one record
 *   (nine sums and the count) per workgroup of 256 pixels in the workspace, added in a fixed order by a second launch -- no atomics.
 *   workspace: pdepth_depth_metrics_workspace_bytes(B, H, W) bytes (80 bytes per 256 pixels), 256-byte aligned; 0 for
 *   non-positive sizes.
 */
size_t pdepth_depth_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pdepth_depth_metrics_f32(const float *logp, const float *pred, const float *d_candi, const float *truth, const float *mask,
                             float clamp_max, int32_t B, int32_t D, int32_t H, int32_t W, float *metrics, float *count,
                             float *depth, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Ground truth from LiDAR: a batch of point clouds -> z-buffered, occlusion-filtered depth maps and masks at full and quarter
 * resolution (generate_depth, external/utils_lib/python/utils_lib.cpp:86-160 with upsample = 0, followed by what the loader does
 * with its result, kittiloader/kitti.py:683-729: util.minpool(large, 4, 1000) and the two masks).
 *   points   [B,Nmax,point_dim] fp32, point_dim 4 = (x, y, z, w) (16-byte aligned) or 3 = (x, y, z) with w = 1;
 *   counts   [B] int32 on the device: rows at or beyond counts[b] are ignored whatever they hold; 0 gives all-zero outputs;
 *   M_velo2cam [4,4] (M_batched = 0) or [B,4,4];  intr [3,4] (intr_batched = 0) or [B,3,4], row-major fp32 (the reference's
 *            binding casts the loader's float64 matrices to fp32 the same way).
 * Per point, fp32, every product and sum rounded on its own, each chain left to right:
 *     cam_r  = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3] w                    r = 0 .. 3
 *     proj_r = ((I[r][0] cam_0 + I[r][1] cam_1) + I[r][2] cam_2) + I[r][3] cam_3      r = 0 .. 2
 *     u_f = proj_0 / proj_2,  v_f = proj_1 / proj_2  (IEEE division);  u = (int)(u_f - 0.5),  v = (int)(v_f - 0.5)
 *   kept iff cam_2 >= 0.1 and finite.  The 0.5 is subtracted in double as the reference does (exact) and the result truncated
 *   toward zero: (-1, 1) is column 0, <= -1 and >= W are outside, likewise v.  A point whose position is not finite or beyond
 *   the int range is skipped (the reference's conversion is undefined there).  The depth is cam_2, not proj_2.
 * Z-buffer: per pixel the minimum cam_2 of the points that land in it (an unsigned atomic minimum on the bit pattern), 0 where
 *   none lands: independent of the order of the points, bit-identical from call to call.
 * Filter (filtering = f in 0 .. 4, filterdiff finite): dmap[v,u] is non-zero only for f <= v < H-f-1 and f <= u < W-f-1 (the
 *   reference's bounds: the last f+1 rows and columns are zero); there it is the z-buffer's z unless another pixel of the
 *   (2f+1)^2 window has zn != 0 and zn - z < -filterdiff (strict; the window reads the z-buffer, never the filtered map).
 * mask = 1.0 where dmap >= 0.01 else 0.0; dmap is multiplied by it.  dmap_quarter [B,H/4,W/4] (a ragged remainder is dropped):
 *   the minimum over 4x4 blocks of dmap with zeros lifted to pool_default (the loader: 1000; 0 = no lifting), a block whose
 *   minimum equals pool_default is 0 -- so a depth >= pool_default beside an empty pixel disappears, as in the reference --;
 *   mask_quarter and the product likewise.  dmap, mask [B,H,W] (16-byte aligned when W % 4 == 0), the quarter outputs may be
 *   NULL when H < 4 or W < 4.
 *   workspace: pdepth_lidar_depth_workspace_bytes(B, H, W) bytes (the z-buffer, 4 H W per item), 256-byte aligned; 0 for
 *   non-positive sizes.  Three launches (clear the z-buffer, a thread per point, a workgroup per 32x32 pixels) on
 *   `stream`: nothing is allocated, nothing waits for the host, the call can be captured in a graph.
 */
size_t pdepth_lidar_depth_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pdepth_lidar_depth_f32(const float *points, const int32_t *counts, const float *M_velo2cam, const float *intr, int32_t B,
                           int32_t Nmax, int32_t point_dim, int32_t M_batched, int32_t intr_batched, int32_t H, int32_t W,
                           int32_t filtering, float filterdiff, float pool_default, float *dmap, float *mask,
                           float *dmap_quarter, float *mask_quarter, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The consistency and smoothness terms of the training loss, one value per batch item, and their gradients (csrc/loss_terms.hip).
 * Each forward is one pass over the maps plus a one-workgroup-per-item sum of the workgroups' partial sums in a fixed order (the
 * same bits from call to call); each backward recomputes the per-pixel quantities from the forward's inputs and scales them by
 * g_value[b] / denominator[b].  Where a mask selects pixels the products with it are kept (x * 0): an item whose mask is empty
 * is 0 / 0 = NaN, and a NaN or an infinite depth makes its own item NaN, as the torch composition does.  Gradient rules are
 * torch's: sign(0) = 0 behind abs, a clamp passes the gradient on min <= x <= max, masks, validity and taps are constants.
 *   All maps fp32, contiguous.  B <= 65535, H, W >= 2 (the down-sample term: >= 4), H * W <= 2^24 (pixel counts are exact in fp32).
 *   workspace: pdepth_loss_terms_workspace_bytes(B, H, W) bytes (8 bytes per 256 pixels and item) for a term whose threads walk
 *   a [B,H,W] map -- the down-sample term walks the small map and needs (B, H/4, W/4) --, 256-byte aligned; 0 for sizes out of range.
 *   value [B]; count [B] = the number of pixels the mask selects (the denominator; the RGB term divides by 3 count).  The backward
 *   entries take the forward's count.  Nothing is allocated, nothing waits for the host.
 *
 * pdepth_loss_dsc_f32: depth_stereo_consistency_loss (losses/loss_blocks.py:147-171 with mean_on_mask :68-71, transform_dmap
 *   utils/inverse_warp.py:212-253, inverse_warp 'nearest' :174-210).  src_depth, tgt_depth, src_mask [B,H,W]; Kinv [B,3,3] and
 *   proj [B,3,4] as pdepth_inverse_warp_f32 takes them (target to source); pose_row = the third row of the 4x4 source-to-target
 *   pose, [B,4] (pose_batched = 1) or [4]; intr [B,3,3].  Per target pixel the sample position, validity and nearest tap are
 *   those of pdepth_inverse_warp_f32 bit for bit; at the tap z = max(src_depth, 1e-3), z' = ((P0 xs z + P1 ys z) + P2 z) + P3 with
 *   xs = (x - cx) / fx, ys = (y - cy) / fy, warped = z' src_mask; m = valid & row >= H / 3 & warped > 0;
 *   value = sum(clamp(|a - b| / |a + b|, 0, 1) m) / sum(m), a = max(tgt_depth m, 1e-3), b = max(warped m, 1e-3).
 *   Backward: g_tgt_depth [B,H,W] through the quotient (written per pixel, reproducible; the nearest warp passes nothing through
 *   the position), g_src_depth [B,H,W] through the tap (cleared, then scattered with float atomics: the last bits depend on the
 *   order of arrival); either may be NULL, not both.
 * pdepth_loss_rsc_f32: rgb_stereo_consistency_loss (losses/loss_blocks.py:114-145).  src_rgb, tgt_rgb [B,3,H,W], tgt_depth
 *   [B,H,W]; bilinear taps with zeros padding, the weights and the fma order of pdepth_inverse_warp_f32; m = valid & row >= H / 3;
 *   value = sum_c sum(|tgt_c m - warped_c m| m) / (3 sum(m)).  Backward: g_tgt_depth [B,H,W] through the sample position -- what
 *   pdepth_inverse_warp_backward_f32 and the products behind it give, in one thread per pixel, no atomics.
 * pdepth_loss_dc_f32: depth_consistency_loss (losses/loss_blocks.py:173-184, minpool utils/img_utils.py:87-95).  large [B,H,W],
 *   small [B,H/4,W/4] (a remainder of H or W is dropped); p = max(min of the 4x4 block, 1e-3) -- a tie goes to the first element
 *   in row-major order --, s = max(small, 1e-3), keep = row >= (H/4) / 3 of the small map;
 *   value = sum(clamp(|p - s| / |p + s|, 0, 1) keep) / sum(keep).  Backward: g_large [B,H,W] (every element written: zero but at the
 *   minimum of each block) and g_small; either may be NULL, not both; no atomics.
 * pdepth_loss_smooth_f32: edge_aware_smoothness_loss at one scale with the image at the map's size (losses/loss_blocks.py:73-112).
 *   depth [B,H,W], rgb [B,3,H,W]; value = mean(|d_y - d_y+1| exp(-mean_c |rgb_y - rgb_y+1|)) + the same along x.  Backward:
 *   g_depth [B,H,W], each pixel gathering its up-to-four differences; no atomics.
 */
size_t pdepth_loss_terms_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pdepth_loss_dsc_f32(const float *src_depth, const float *tgt_depth, const float *src_mask, const float *Kinv, const float *proj,
                        const float *pose_row, int32_t pose_batched, const float *intr, int32_t B, int32_t H, int32_t W,
                        float *value, float *count, void *workspace, size_t workspace_bytes, void *stream);
int pdepth_loss_dsc_backward_f32(const float *src_depth, const float *tgt_depth, const float *src_mask, const float *Kinv,
                                 const float *proj, const float *pose_row, int32_t pose_batched, const float *intr,
                                 const float *count, const float *g_value, int32_t B, int32_t H, int32_t W, float *g_src_depth,
                                 float *g_tgt_depth, void *stream);
int pdepth_loss_rsc_f32(const float *src_rgb, const float *tgt_rgb, const float *tgt_depth, const float *Kinv, const float *proj,
                        int32_t B, int32_t H, int32_t W, float *value, float *count, void *workspace, size_t workspace_bytes,
                        void *stream);
int pdepth_loss_rsc_backward_f32(const float *src_rgb, const float *tgt_rgb, const float *tgt_depth, const float *Kinv,
                                 const float *proj, const float *count, const float *g_value, int32_t B, int32_t H, int32_t W,
                                 float *g_tgt_depth, void *stream);
int pdepth_loss_dc_f32(const float *large, const float *small, int32_t B, int32_t H, int32_t W, float *value, float *count,
                       void *workspace, size_t workspace_bytes, void *stream);
int pdepth_loss_dc_backward_f32(const float *large, const float *small, const float *count, const float *g_value, int32_t B,
                                int32_t H, int32_t W, float *g_large, float *g_small, void *stream);
int pdepth_loss_smooth_f32(const float *depth, const float *rgb, int32_t B, int32_t H, int32_t W, float *value, void *workspace,
                           size_t workspace_bytes, void *stream);
int pdepth_loss_smooth_backward_f32(const float *depth, const float *rgb, const float *g_value, int32_t B, int32_t H, int32_t W,
                                    float *g_depth, void *stream);

/*
 * Deterministic backward: the three scattered gradients as order-independent sums.
 *
 * grad_src of pdepth_sweep_backward_f32, g_src_depth of pdepth_loss_dsc_backward_f32 and grad_img of
 * pdepth_inverse_warp_backward_f32 are sums of contributions that arrive in an order the hardware chooses; with float atomics
 * their last bits differ from call to call.  The _det entries below form the same contributions q_i (the same fp32 expressions
 * in the same order as the entries they stand beside) and sum them exactly, as integers:
 *     g[t] = fl32(2^-S_b sum_i rn(2^S_b q_i)),     rn: to the nearest integer, ties to even; the product is exact (formed in double)
 * added with 64-bit integer atomics into an accumulator in the workspace and converted by a last pass.  The result depends only
 * on the multiset of contributions: two calls give the same bits, and so do two builds that stage or group the adds differently.
 *
 * The scale: S_b is chosen per batch item b, on the device (no read-back, no host synchronisation), so an item's result does not
 * depend on the other items of the batch.  With M_b a bound of |q_i| over the item and N the largest number of contributions one
 * destination can receive, S_b = pdepth_det_scale_exponent(M_b, N): the integer with N 2 M_b 2^S_b <= 2^62 (no overflow of the
 * int64, roundings included) and N M_b 2^S_b > 2^58 (at most 3 of the 62 bits unused); every contribution is thus rounded at
 * 2^-59 N M_b or finer.
 *   sweep:  N = D H W (per view a (plane, pixel) sample puts at most one tap, of weight <= 1, on a texel);
 *           M_b = |gscale| max|grad_cost[b]| E_b, gscale = 2 / sigma (L2), 1 / sigma (L1), E_b = max|src[b]| + max|ref[b]| (L2), 1 (L1),
 *           the maxima from a pre-pass over the item's inputs;
 *   dsc, inverse_warp:  N = 4 H W (pixels x taps); M_b = the exact maximum of |q_i|, from a first run of the per-pixel chain.
 *   warp_feature (the fourth case, further below):  N = H W, M_b likewise;
 *   flow_warp (the fifth: grad_x of pdepth_flow_warp_backward_f32, declared with the flow entries below):  N = 4 H W, M_b likewise.
 * M_b == 0: the item's gradient is exactly 0.
 * Non-finite: if M_b is NaN or infinite -- a NaN or an infinity among the inputs that enter it --, or overflows (the sweep: M_b or
 * one of its factors |gscale| max|grad_cost[b]|, E_b at or above 2^127, where the fp32 chain may leave the finite range), EVERY
 * element of that item's scattered gradient is NaN, and every other item is untouched.  This departs on purpose from the atomic
 * entries, which confine a NaN to the texels it reaches: an integer accumulator cannot hold a NaN, and a non-finite gradient
 * anywhere in an item is what an overflow check of a loss scaler looks for.
 * Conversion: int64 -> double (exact below 2^53, else one rounding to nearest), times 2^-S_b (exact), double -> fp32 (one rounding
 * to nearest): at most two roundings, always the same instruction sequence.
 * The gradients written per owner (grad_ref, g_tgt_depth, grad_point) come from the kernels of the atomic entries and have the
 * same bits as theirs.
 *
 * Workspace (256-byte aligned; needed when the scattered gradient is requested; cleared by the call):
 *   sweep         roundup256(16 B) + roundup256(8 B V C H W) bytes: B = 4, V = 1, C = 67: 17.6 MB at 64 x 128, 281 MB at 256 x 512;
 *   dsc           roundup256(4 B)  + roundup256(8 B H W);
 *   inverse_warp  roundup256(4 B)  + roundup256(8 B C H W);
 *   flow_warp     roundup256(4 B)  + roundup256(8 B C H W).
 * The queries return 0 for sizes out of range.  A workspace that is missing, too small or misaligned is PDEPTH_E_WORKSPACE.
 *
 * pdepth_det_scale_exponent(bound, n): the exponent rule itself, a host function (the kernels call the same inline code): S for
 * a finite bound > 0 (denormals included) and n >= 1; PDEPTH_DET_EXP_ZERO for bound == 0; PDEPTH_DET_EXP_NONFINITE for a NaN or
 * infinite bound (or n < 1).
 * Every other argument, check and message: as the entry without _det.
 */
#define PDEPTH_DET_EXP_ZERO (-2147483647 - 1)
#define PDEPTH_DET_EXP_NONFINITE 2147483647
int32_t pdepth_det_scale_exponent(float bound, int64_t n);
size_t pdepth_sweep_backward_det_workspace_bytes(const pdepth_sweep_desc *desc);
int pdepth_sweep_backward_det_f32(const pdepth_sweep_desc *desc, const pdepth_camera *cam, const float *ref, const float *src,
                                  const float *d_candi, const float *grad_cost, float *grad_ref, float *grad_src, void *workspace,
                                  size_t workspace_bytes, void *stream);
size_t pdepth_loss_dsc_backward_det_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pdepth_loss_dsc_backward_det_f32(const float *src_depth, const float *tgt_depth, const float *src_mask, const float *Kinv,
                                     const float *proj, const float *pose_row, int32_t pose_batched, const float *intr,
                                     const float *count, const float *g_value, int32_t B, int32_t H, int32_t W, float *g_src_depth,
                                     float *g_tgt_depth, void *workspace, size_t workspace_bytes, void *stream);
size_t pdepth_inverse_warp_backward_det_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int pdepth_inverse_warp_backward_det_f32(const float *img, const float *depth, const float *Kinv, const float *proj,
                                         const float *grad_out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t mode,
                                         float *grad_img, float *grad_point, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward of pdepth_warp_feature_f32 with respect to src: the fourth scattered gradient, in both forms.
 *
 * The forward is linear in src: out[b,v,k,y,x] = bilinear(src[b,v,k], pos_k(b,v,y,x)), zeros padding, align_corners=False, channel k
 * sampled at plane k.  Nothing of it is saved:
 *     grad_src[b,v,k,t] = sum over the samples (y,x) of grad_out[b,v,k,y,x] w_tap(t),   over the at most 4 in-bounds taps of each.
 * Positions, taps and weights are the forward's, bit for bit (one per-sample chain for both kernels).  The taps follow ATen's
 * grid_sampler_2d backward: an in-bounds tap receives g w even when w == 0 (an infinite g leaves a NaN there), an out-of-bounds tap
 * receives nothing, and a non-finite position has no tap.
 *
 * desc is read as pdepth_warp_feature_f32 reads it (C == D planes, algo, blas_mode); src_vstride = D H W and src_bstride = V D H W
 * describe grad_src, which must be contiguous [B,V,D,H,W], as grad_out is.  D <= 512, H W <= 2^30, B <= 65535; grad_src may not
 * alias grad_out.
 *   pdepth_warp_feature_backward_f32      float atomics into grad_src (zeroed by the call on the stream, by a launch): the last bits depend on
 *                                         the order in which the adds arrive; a non-finite grad_out stays in the texels it reaches.
 *   pdepth_warp_feature_backward_det_f32  the order-independent sum described above: q_i = g w_tap, M_b = the exact maximum of
 *                                         |q_i| over item b (a first run of the chain), N = H W (a sample puts at most one of its
 *                                         taps on a texel of its own (b,v,k) image).  M_b == 0: the item is exactly 0.  A NaN or
 *                                         an infinity among the q_i of an item: NaN in EVERY element of that item, every other
 *                                         item untouched.
 *                                         Workspace: roundup256(4 B) + roundup256(8 B V D H W) bytes, 256-byte aligned, cleared by
 *                                         the call (B = 4, V = 2, D = 64, 64 x 128: 33.6 MB); the query returns 0 for sizes out of
 *                                         range; missing, too small or misaligned: PDEPTH_E_WORKSPACE.
 */
int pdepth_warp_feature_backward_f32(const pdepth_sweep_desc *desc, const pdepth_camera *cam, const float *d_candi,
                                     const float *grad_out, float *grad_src, void *stream);
size_t pdepth_warp_feature_backward_det_workspace_bytes(const pdepth_sweep_desc *desc);
int pdepth_warp_feature_backward_det_f32(const pdepth_sweep_desc *desc, const pdepth_camera *cam, const float *d_candi,
                                         const float *grad_out, float *grad_src, void *workspace, size_t workspace_bytes,
                                         void *stream);

/*
 * SSIM distance between two images and its gradients (csrc/ssim.hip): SSIM(x, y, md) of losses/loss_blocks.py:47-66, the
 * photometric term of losses/flow_loss.py:13-27.
 *
 * x, y [B,C,H,W] fp32 contiguous -> out [B,C,H-2md,W-2md], md = 1, 2 or 3, one value per window of n = (2 md + 1)^2 pixels (valid
 * windows only, as AvgPool2d(2 md + 1, 1, 0) places them).  Per window, with the sums divided by n:
 *     s_x = e_xx - m_x^2,  s_y = e_yy - m_y^2,  s_xy = e_xy - m_x m_y,
 *     A1 = 2 m_x m_y + C1,  A2 = 2 s_xy + C2,  B1 = m_x^2 + m_y^2 + C1,  B2 = s_x + s_y + C2,   C1 = 1e-4, C2 = 9e-4,
 *     S = A1 A2 / (B1 B2),   out = clamp((1 - S) / 2, 0, 1).
 * fp32 throughout, one rounding per operation, each window sum one running sum over its pixels in row-major order (the order of
 * ATen's average pooling): the same bits from call to call.  The form is the reference's symmetric one: where x and y are equal bit for bit, out is
 * exactly 0.  A NaN stays a NaN through the clamp.
 *
 * Backward: g_out [B,C,H-2md,W-2md] -> g_x, g_y [B,C,H,W]; either may be NULL, not both, and a NULL one is not stored.  The clamp
 * passes the gradient on 0 <= (1 - S) / 2 <= 1, both edges included (torch.clamp's rule): a window that sits exactly on an edge
 * -- two all-zero patches, S == 1 -- passes it.  Nothing of the forward is kept: each window's chain is recomputed from x and y,
 * with the forward's bits, and every pixel gathers the (2 md + 1)^2 windows that contain it in a fixed order.  No atomics: two
 * calls give the same bits, and a call for one gradient gives the bits of the call for both.  Where x and y are equal bit for bit
 * both gradients are exactly 0.  The outputs may not alias each other or an input.
 *
 * B * C <= 65535 (a plane per grid z), H, W >= 2 md + 1, H * W <= 2^30, H <= 1048560; md outside 1..3: PDEPTH_E_ARG.  One launch
 * each on `stream`; nothing is allocated, nothing waits for the host.
 */
int pdepth_ssim_f32(const float *x, const float *y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t md, float *out, void *stream);
int pdepth_ssim_backward_f32(const float *x, const float *y, const float *g_out, int32_t B, int32_t C, int32_t H, int32_t W,
                             int32_t md, float *g_x, float *g_y, void *stream);

/*
 * The photometric term in one pass each way (csrc/photo.hip): the bilinear warp of pdepth_loss_rsc_f32, its masked L1 distance and
 * the SSIM distance of the masked images, per batch item -- rgb_stereo_consistency_loss (losses/loss_blocks.py:114-145) with the
 * SSIM it carries commented out (:128-129) mixed in as the flow loss mixes it (losses/flow_loss.py:13-27).
 *
 * src_rgb, tgt_rgb [B,3,H,W], tgt_depth [B,H,W], Kinv [B,3,3], proj [B,3,4] as pdepth_loss_rsc_f32 takes them.  With
 * m = valid & row >= H / 3 (the bits of pdepth_inverse_warp_f32's `valid`), x = warped m, y = tgt m, md = 1, 2 or 3,
 * n_w = 3 (H - 2 md)(W - 2 md) and S the SSIM of pdepth_ssim_f32 over (x, y), in that order:
 *     value = (1 - w) sum_c sum(|y_c - x_c| m) / (3 sum(m))  +  w (sum_windows clamp((1 - S) / 2, 0, 1) / n_w) / (sum(m) / (H W))
 *     count = sum(m)
 * w = ssim_weight, a double as the Python number it comes from: the factors are (float)w and (float)(1 - w), the difference taken
 * in double, as torch forms them.  A window has the bits it has in pdepth_ssim_f32 on the same x and y.  The products with the mask
 * stay products: a NaN behind a zero mask makes its item NaN; an empty mask is 0 / 0 = NaN for its item alone.
 * Forward: one launch (a workgroup per 64 x 16 tile of an item; nothing per-pixel is written) and the sum of the workgroups' three
 * partial sums per item in a fixed order, in double.  No atomics: two calls give the same bits.
 *   workspace: pdepth_loss_photo_workspace_bytes(B, H, W) bytes (12 bytes per tile and item), 256-byte aligned; 0 for sizes out of
 *   range.  A workspace that is missing, too small or misaligned is PDEPTH_E_WORKSPACE.
 * Backward: g_tgt_depth [B,H,W] and nothing else, in one launch that recomputes from the inputs; it takes the forward's count, which
 * like the mask mean is a constant of the gradient.  Per pixel p and channel c, with d_c = y_c - x_c and n = (2 md + 1)^2:
 *     g_warped_c = -(1 - w) g / (3 count) sign0(d_c) m  +  m sum_{windows containing p} (P + Q x_p + R y_p) / n
 * P, Q, R the coefficients of pdepth_ssim_backward_f32 with G = -1/2 g w / (n_w count / (H W)) on the windows that pass the clamp
 * (0 <= (1 - S) / 2 <= 1, both edges included) and 0 elsewhere; then through the sample position as pdepth_loss_rsc_backward_f32.
 * Every pixel gathers its windows in a fixed order: two calls give the same bits.
 * B <= 65535, H, W >= 2 md + 1, H * W <= 2^24, H <= 1048560; md outside 1..3: PDEPTH_E_ARG.  Nothing is allocated, nothing waits
 * for the host.
 */
size_t pdepth_loss_photo_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pdepth_loss_photo_f32(const float *src_rgb, const float *tgt_rgb, const float *tgt_depth, const float *Kinv, const float *proj,
                          int32_t B, int32_t H, int32_t W, double ssim_weight, int32_t md, float *value, float *count,
                          void *workspace, size_t workspace_bytes, void *stream);
int pdepth_loss_photo_backward_f32(const float *src_rgb, const float *tgt_rgb, const float *tgt_depth, const float *Kinv,
                                   const float *proj, const float *count, const float *g_value, int32_t B, int32_t H, int32_t W,
                                   double ssim_weight, int32_t md, float *g_tgt_depth, void *stream);

/*
 * Ternary census distance between two RGB images and its gradients (csrc/ternary.hip): TernaryLoss(im, im_warp, max_distance) of
 * losses/loss_blocks.py:8-44, the third photometric piece of losses/flow_loss.py:13-27.
 *
 * x, y [B,3,H,W] fp32 contiguous -> out [B,1,H,W], md = 1, 2 or 3, K = 2 md + 1.  With I = ((0.2989 r + 0.5870 g) + 0.1140 b) 255
 * of x and I' of y, and per offset o of the K x K patch
 *     t = I(p+o) - I(p)    n = t / sqrt(0.81 + t^2)    (n' from I')    d = (n - n')^2    h = d / (0.1 + d)
 * out(p) = (sum_o h) / K^2 where p is at least md from every border, and 0 elsewhere: no output that is kept reads outside the
 * image.  Square roots and divisions are correctly rounded and nothing is contracted, so n, d and h have the bits of the float32
 * reference; the sum runs over the offsets rows first.  Where x and y are equal bit for bit, out is exactly 0.
 * Backward: g_out [B,1,H,W] -> g_x, g_y [B,3,H,W]; either may be NULL (not computed), not both.  With G = g_out / K^2 on the
 * pixels at least md from every border and 0 elsewhere (outside the image too), and h's derivatives being odd in (t, t'),
 *     g_I(p) = -sum_o (G(p) + G(p+o)) dh/dt,     dh/dt = a 0.81 / s^3,  dh/dt' = -a 0.81 / s'^3,  a = 0.2 (n - n') / (0.1 + d)^2,
 * s = sqrt(0.81 + t^2); g_x = g_I 255 (0.2989, 0.5870, 0.1140), likewise g_y from I'.  Every pixel of the image gets a gradient,
 * the border ring included (its pixels are neighbours of interior ones).  A gather that recomputes from the inputs, in a fixed
 * order, no atomics: two calls give the same bits; where x and y are equal bit for bit both gradients are exactly 0.
 *
 * B <= 65535 (an item per grid z), H, W >= 2 md + 1, H * W <= 2^30, H <= 524280; md outside 1..3: PDEPTH_E_ARG; the outputs may
 * not alias each other or an input.  One launch each on `stream`; nothing is allocated, nothing waits for the host.
 */
int pdepth_ternary_f32(const float *x, const float *y, int32_t B, int32_t H, int32_t W, int32_t md, float *out, void *stream);
int pdepth_ternary_backward_f32(const float *x, const float *y, const float *g_out, int32_t B, int32_t H, int32_t W, int32_t md,
                                float *g_x, float *g_y, void *stream);

/*
 * Range map of a forward splat and the occlusion mask behind it (csrc/occlusion.hip): get_corresponding_map (utils/warp_utils.py:
 * 25-79) and 1 - get_occu_mask_backward (:102-108), the third operand of the photometric composition of losses/flow_loss.py:72-78.
 *
 *     range[b,y,x] = sum over the source pixels p of the bilinear weight with which p's position lands on (x, y)
 *     visible      = (min(max(range, 0), 1) < th) ? 0 : 1                                  (1 = some source pixel sees it)
 * Only in-bounds taps count; a NaN or infinite position adds nothing.  Two forms of the position:
 *   pdepth_range_map_f32        coords [B,2,H,W]: un-normalised (x, y) per source pixel.  With w = x - floor(x), e = 1 - w and n, s
 *                               likewise from y, the taps (floor x, floor y) ... (+1, +1) receive s e, s w, n e, n w: fp32, one
 *                               rounding per operation.
 *   pdepth_depth_range_map_f32  depth [B,H,W] of the source view, src_mask [B,H,W] or NULL (a pixel whose mask is 0 adds nothing),
 *                               Kinv [B,3,3], proj [B,3,4]: the position is the one pdepth_inverse_warp_f32 samples pixel (x, y) at
 *                               with these matrices and this depth, bit for bit -- its align_corners=False un-normalisation of
 *                               cam2pixel's 2 X / (W - 1) - 1 included, so the mask describes the warp the opposite term performs.
 * range and visible are [B,1,H,W]; either may be NULL (not written), not both.
 *
 * The sum is an order-independent integer sum (pdepth_det_scale_exponent(1, H W): every weight lies in [0, 1] and a destination
 * receives at most one tap per source pixel, so no maximum pass is needed): the same bits from call to call and on any stream, and
 * an item's result does not depend on its neighbours in the batch.  A destination's error is below (1 + its contributions) 2^-22
 * against the float64 sum over the same fp32 positions.  There is no float-atomics variant: a mass within an ulp of th would flip a
 * mask bit with the order of arrival.
 *
 * Workspace: roundup256(8 B H W) bytes, 256-byte aligned, cleared by the call; the query returns 0 for sizes out of range; missing,
 * too small or misaligned: PDEPTH_E_WORKSPACE.  H * W <= 2^24, B <= 65535, H, W >= 1 (the depth form: >= 2); a null input, no
 * output, a non-positive size or th NaN: PDEPTH_E_ARG, before any launch.  Three launches on `stream` (the zero fill of the
 * workspace is a kernel: the call can be captured in a graph and replayed); nothing is allocated, nothing waits for the host.
 */
size_t pdepth_range_map_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pdepth_range_map_f32(const float *coords, int32_t B, int32_t H, int32_t W, float th, float *range, float *visible,
                         void *workspace, size_t workspace_bytes, void *stream);
int pdepth_depth_range_map_f32(const float *depth, const float *src_mask, const float *Kinv, const float *proj, int32_t B, int32_t H,
                               int32_t W, float th, float *range, float *visible, void *workspace, size_t workspace_bytes,
                               void *stream);

/*
 * flow_warp and the forward-backward check of the unsupervised flow loss (csrc/flow_warp.hip): utils/warp_utils.py:82-99 over
 * F.grid_sample, bilinear, align_corners=False; the operands of losses/flow_loss.py:66-78.
 *
 * x [B,C,H,W] is sampled at base grid + flow [B,2,H,W] (channel 0 along x); pad: 0 = border, 1 = zeros.  The chain of pixel
 * (row y, column x) (csrc/flow_warp_sample.hpp, run by every kernel of these entries): the position is formed in double from the
 * fp32 flow, and only its fractions are rounded to fp32 --
 *     vx = double(x) + double(flow[b,0,y,x])   (exact)        ix = vx (double(W) / double(W - 1)) - 0.5
 * and likewise iy: the reference's mixed normalisation, 2 v / (W - 1) - 1 un-normalised by ((g + 1) W - 1) / 2, as the number it
 * defines (the reference's own fp32 chain rounds the normalised coordinate near 1 and is about W / 2 eps32 from that number
 * everywhere in the image: 2.5e-5 px at W = 832; the double operations are per pixel, not per channel).  Border: ix is clamped to
 * [0, W - 1], iy to [0, H - 1].  x0 = floor(ix), x1 = x0 + 1; w = ix - x0, e = x1 - ix, n = iy - y0, s = y1 - iy, each rounded to
 * fp32 once; from there fp32, one rounding per operation and no fma: the taps (x0, y0), (x1, y0), (x0, y1), (x1, y1) weigh e s,
 * w s, e n, w n; each tap is tested for bounds on its own and an out-of-bounds tap contributes 0 (border at ix = W - 1: the x1
 * column is outside, with weight 0).  out = ((v_nw nw + v_ne ne) + v_sw sw) + v_se se.
 * A position that is not finite before the clamp has no tap and gives 0 in BOTH paddings, value and gradients -- a stated
 * departure: ATen's clamp of a NaN is unspecified, and it clamps an infinite position to the border.
 *
 *   pdepth_flow_warp_f32               out [B,C,H,W].  One launch.
 *   pdepth_flow_warp_backward_f32      grad_x [B,C,H,W] and grad_flow [B,2,H,W]; either may be NULL, not both.
 *       grad_flow is written per owner, one thread summing d out / d (ix, iy) grad_out over the channels of its pixel in channel
 *       order: no atomics, the same bits from call to call.  d ix / d flow_x = (W / 2) (2 / (W - 1)); with border padding the factor
 *       is 0 where the position was clamped from strictly outside [0, W - 1] and 1 at exactly 0 or W - 1 (likewise y).
 *       grad_x is a scatter of g w_tap: an in-bounds tap receives g w even when w == 0, an out-of-bounds tap nothing (the rules
 *       of pdepth_warp_feature_backward_f32); float atomics into grad_x, zeroed by the call on the stream, by a launch.
 *   pdepth_flow_warp_backward_det_f32  grad_x as the order-independent sum of "Deterministic backward" above: its fifth case,
 *       q_i = g w_tap, N = 4 H W, M_b the exact maximum of |q_i| over item b (a first run of the chain); M_b == 0, NaN and overflow
 *       as the other _det entries.  grad_flow has the bits of the atomic entry.  Workspace: roundup256(4 B) + roundup256(8 B C H W)
 *       bytes, 256-byte aligned, needed when grad_x is requested, cleared by the call; the query returns 0 for sizes out of range;
 *       missing, too small or misaligned: PDEPTH_E_WORKSPACE.
 *   pdepth_flow_fb_check_f32           occ [B,1,H,W] = 1.0 where |flow12 + w|^2 > scale (|flow12|^2 + |w|^2) + bias, else 0.0, with
 *       w the two channels of flow21 sampled at base + flow12 with zeros padding by the chain above; |a|^2 = a_x a_x + a_y a_y,
 *       the right side (|flow12|^2 + |w|^2) scale + bias, fp32.  One launch; a mask has no gradient.
 * B <= 65535, H, W >= 2 (the reference divides by H - 1 and W - 1), H * W <= 2^30; a null pointer, a non-positive size, H or W
 * below 2, an unknown pad, no gradient requested, a NaN scale or bias: PDEPTH_E_ARG, before any launch.  Nothing is allocated,
 * nothing waits for the host.
 */
int pdepth_flow_warp_f32(const float *x, const float *flow, int32_t B, int32_t C, int32_t H, int32_t W, int32_t pad, float *out,
                         void *stream);
int pdepth_flow_warp_backward_f32(const float *x, const float *flow, const float *grad_out, int32_t B, int32_t C, int32_t H,
                                  int32_t W, int32_t pad, float *grad_x, float *grad_flow, void *stream);
size_t pdepth_flow_warp_backward_det_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int pdepth_flow_warp_backward_det_f32(const float *x, const float *flow, const float *grad_out, int32_t B, int32_t C, int32_t H,
                                      int32_t W, int32_t pad, float *grad_x, float *grad_flow, void *workspace,
                                      size_t workspace_bytes, void *stream);
int pdepth_flow_fb_check_f32(const float *flow12, const float *flow21, int32_t B, int32_t H, int32_t W, float scale, float bias,
                             float *occ, void *stream);

/*
 * First-order smoothness of a flow (csrc/loss_smooth1.hip): smooth_grad_1st of losses/loss_blocks.py:210-220, the smoothness term
 * of losses/flow_loss.py:29-32.  flo [B,Cf,H,W], image [B,Ci,H,W], one value for the batch:
 *     wx = exp(-alpha mean_c |image[..., x+1] - image[..., x]|),   value = mean(wx |dx flo|) / 4 + mean(wy |dy flo|) / 4
 * the means over [B,Cf,H,W-1] and [B,Cf,H-1,W].  fp32 per pair (the channel sum in channel order), a workgroup's 256 pixels summed
 * in a fixed tree, the workgroups' sums added in a fixed order in double: the same bits from call to call.  value is ONE float.
 * Workspace: pdepth_loss_terms_workspace_bytes(B, H, W).  Backward: g_value [1] -> g_flo [B,Cf,H,W], every flow value gathering
 * its left / right and up / down differences, sign(0) = 0; no atomics.  image is data.  H, W >= 2, H * W <= 2^24, B <= 65535.
 */
int pdepth_loss_smooth1_f32(const float *flo, const float *image, int32_t B, int32_t Cf, int32_t Ci, int32_t H, int32_t W,
                            float alpha, float *value, void *workspace, size_t workspace_bytes, void *stream);
int pdepth_loss_smooth1_backward_f32(const float *flo, const float *image, const float *g_value, int32_t B, int32_t Cf, int32_t Ci,
                                     int32_t H, int32_t W, float alpha, float *g_flo, void *stream);

/*
 * The per-level cost volume of the flow network (csrc/cost_volume.hip; models/pwclite.py: flow_warp, the correlation, LeakyReLU)
 * in one pass:
 *     out = leaky_relu(correlation(x1, flow_warp(x2, flow, pad)), negative_slope)          [B, (2 md + 1)^2, H, W],  md = max_displacement
 * x1, x2 [B,C,H,W], flow [B,2,H,W] or NULL (no warp: the network's coarsest level; still one launch), fp32.  The correlation is the
 * configuration the reference instantiates: kernel 1, both strides 1, pad_size = max_displacement,
 *     out[b, (tj + md)(2 md + 1) + (ti + md), y, x] = (1 / C) sum_c x1[b,c,y,x] w[b,c,y+tj,x+ti]     (tj the row displacement)
 * with w the warped x2 and zeros outside the image.  A warped texel is the chain of the flow entries above
 * (csrc/flow_warp_sample.hpp: the position formed in double; a non-finite position gives 0 in both paddings).  The sum runs over c
 * in ascending order in fp32 (blocks of 8 channels: a block's sum by one fma per channel, the blocks' sums added in turn), then
 * times 1 / C, then x > 0 ? x : x negative_slope.  The zeros of the correlation's
 * padding are multiplied, not skipped: 0 x inf gives NaN, as in pdepth_correlation_forward_f32.  Neither the warped image nor the
 * pre-activation volume reaches global memory.
 *
 *   pdepth_flow_cost_volume_f32               out.  One launch.
 *   pdepth_flow_cost_volume_backward_f32      grad_x1 [B,C,H,W], grad_x2 [B,C,H,W], grad_flow [B,2,H,W]; any may be NULL, not all three
 *       (grad_flow must be NULL without a flow).  `out` is the forward's saved result: the activation's factor is
 *       out > 0 ? 1 : negative_slope (0, -0 and NaN take the slope); no pre-activation is kept.  Launch 1 gathers, without atomics,
 *       grad_x1 and the gradient of the warped image into the workspace; launch 2 is pdepth_flow_warp_backward_f32's own work on that
 *       gradient: grad_x2 by float atomics (zeroed by the call on the stream, by a launch), grad_flow per owner.  Without a flow the gradient of
 *       the "warped" image is grad_x2 itself: one launch, no workspace.
 *   pdepth_flow_cost_volume_backward_det_f32  grad_x2 by the order-independent sum of pdepth_flow_warp_backward_det_f32 (the fifth
 *       case of "Deterministic backward" above); everything else has the bits of the entry without _det.
 * Workspace with a flow (256-byte aligned; needed when grad_x2 or grad_flow is requested): roundup256(4 B C H W) bytes; _det, when
 * grad_x2 is requested: that plus the bytes of pdepth_flow_warp_backward_det_workspace_bytes(B, C, H, W).  The queries take
 * with_flow (0: no flow, no workspace) and return 0 for sizes out of range.  Missing, too small or misaligned: PDEPTH_E_WORKSPACE.
 * max_displacement in 1..4; H, W >= 2 with a flow (>= 1 without); H * W <= 2^30, H <= 16 * 65535, B * ceil(C / 8) <= 65535; pad as
 * the flow entries; a NaN or negative negative_slope, a null pointer, no gradient requested: PDEPTH_E_ARG, before any launch.
 * Nothing is allocated, nothing waits for the host.
 */
int pdepth_flow_cost_volume_f32(const float *x1, const float *x2, const float *flow, int32_t B, int32_t C, int32_t H, int32_t W,
                                int32_t max_displacement, float negative_slope, int32_t pad, float *out, void *stream);
size_t pdepth_flow_cost_volume_backward_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t with_flow);
int pdepth_flow_cost_volume_backward_f32(const float *x1, const float *x2, const float *flow, const float *out, const float *grad_out,
                                         int32_t B, int32_t C, int32_t H, int32_t W, int32_t max_displacement, float negative_slope,
                                         int32_t pad, float *grad_x1, float *grad_x2, float *grad_flow, void *workspace,
                                         size_t workspace_bytes, void *stream);
size_t pdepth_flow_cost_volume_backward_det_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t with_flow);
int pdepth_flow_cost_volume_backward_det_f32(const float *x1, const float *x2, const float *flow, const float *out,
                                             const float *grad_out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t max_displacement,
                                             float negative_slope, int32_t pad, float *grad_x1, float *grad_x2, float *grad_flow,
                                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * One direction of the photometric term of the unsupervised flow loss in one pass each way (csrc/flow_photo.hip):
 * losses/flow_loss.py:13-27, loss_photomatric at its fixed max_distance = 1, with the warp of :66-78 inside.  im, other [B,3,H,W],
 * flow [B,2,H,W], mask [B,1,H,W] (any float; in practice 0 / 1), pad as the flow entries.  With R = flow_warp(other, flow, pad) by the
 * chain of pdepth_flow_warp_f32 (the same bits), x = R mask, y = im mask and N = B H W:
 *     value = ( w_l1 sum |im - R| mask / (3 N)  +  w_ssim sum_windows dist(x, y) / (3 B (H - 2)(W - 2))  +  w_ternary sum T(x, y) / N )
 *             / (sum(mask) / N)
 *     count = sum(mask)
 * dist the clamped 3 x 3 window distance of pdepth_ssim_f32 (md = 1), T the census distance of pdepth_ternary_f32 (md = 1; 0 in the
 * border ring; its zero padding sees the masked images).  value and count are ONE float each.  A weight that is not > 0 -- zero,
 * negative, NaN: the reference's `if w > 0` -- removes its term entirely: nothing of it is evaluated, a NaN it would have produced
 * does not reach the value; with all three off the value is 0 / (sum(mask) / N).  The products with the mask stay products: a NaN
 * behind a zero mask makes the value NaN; sum(mask) == 0 gives 0 / 0 = NaN; a non-finite flow has no tap and R = 0 there.
 *
 *   pdepth_flow_photo_f32           two launches: a workgroup per 64 x 8 tile and item evaluates the warp chain for the tile and a
 *       halo of 1 and writes four partial sums (fp32, a fixed tree) to the workspace; one workgroup adds them in a fixed order in
 *       double.  No atomics: the same bits from call to call.  Nothing per-pixel is written.
 *   pdepth_flow_photo_backward_f32  count [1] (the forward's), g_value [1] -> g_flow [B,2,H,W], one launch; the images and the mask
 *       are data.  The chain is recomputed with a halo of 2.  Per pixel and channel the gradient of R is the sum of
 *       -g w_l1 / (3 N) sign(im - R) mask (sign(0) = 0), mask times the gather of pdepth_ssim_backward_f32 over the up to nine windows
 *       that contain the pixel (in its order, with the forward's clamp decision, inclusive rule), and mask 255 (0.2989, 0.5870,
 *       0.1140)_c times the census gather of pdepth_ternary_backward_f32, with g = g_value / (count / N); g_flow is formed from it as
 *       pdepth_flow_warp_backward_f32 forms grad_flow (channel order, the clamp factors).  A gather in a fixed order: no atomics, the
 *       same bits from call to call.
 * Workspace: pdepth_flow_photo_workspace_bytes(B, H, W) = roundup256(16 ceil(W / 64) ceil(H / 8) B) bytes, 256-byte aligned; the
 * query returns 0 for sizes out of range; missing, too small or misaligned: PDEPTH_E_WORKSPACE.
 * The sizes and pads pdepth_flow_warp_f32 refuses are refused; B * H * W <= 2^24 (a pixel count is exact in fp32); H and W of at least
 * 3 when w_ssim or w_ternary is on (the message names "H=.., W=.."); a null pointer, g_flow aliasing flow: PDEPTH_E_ARG, before any
 * launch.  Nothing is allocated, nothing waits for the host.
 */
size_t pdepth_flow_photo_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pdepth_flow_photo_f32(const float *im, const float *other, const float *flow, const float *mask, int32_t B, int32_t H, int32_t W,
                          int32_t pad, double w_l1, double w_ssim, double w_ternary, float *value, float *count, void *workspace,
                          size_t workspace_bytes, void *stream);
int pdepth_flow_photo_backward_f32(const float *im, const float *other, const float *flow, const float *mask, const float *count,
                                   const float *g_value, int32_t B, int32_t H, int32_t W, int32_t pad, double w_l1, double w_ssim,
                                   double w_ternary, float *g_flow, void *stream);

/*
 * Optical-flow evaluation: end-point error means, the KITTI outlier rate ("Fl") and the mask sums per item of a batch, on the
 * device (utils/flow_utils.py:61-123 evaluate_flow, which copies the prediction to the host, rescales it, resizes it with
 * cv2.resize and loops over the items; its callers: trainer/sintel_trainer.py:92-151).
 *   gt        [B,gt_channels,H,W]: gt_channels 2 = (u, v), or 4 = (u, v, valid, noc) as the KITTI loaders stack them;
 *   pred      [B,2,h,w], h and w any size (larger, smaller or equal, each axis on its own);
 *   move_mask [B,H,W] or NULL, with gt_channels == 4 only.
 * Per item b and ground-truth pixel (y, x):
 *     u' = (u / (float)w) * (float)W,  v' = (v / (float)h) * (float)H         the reference's two float operations, in its order
 *                                                                            (flow_utils.py:77-80), applied to each tap
 *     (up, vp) = the bilinear sample of (u', v') under cv2.resize's INTER_LINEAR rule: half-pixel centres,
 *                sx = (x + 0.5) w / W - 0.5, x0 = floor(sx); x0 < 0: tap 0 with weight 1; x0 >= w - 1: tap w - 1 with weight 1;
 *                otherwise taps x0, x0 + 1 with weights 1 - (sx - x0), sx - x0; rows alike; the two rows are interpolated first,
 *                then the column; no antialiasing when shrinking (in exact arithmetic: F.interpolate(mode='bilinear',
 *                align_corners=False)).  The position is formed in double, the weights and the sums of products in float.
 *     epe = sqrtf((up - gu)^2 + (vp - gv)^2)
 *     bad(m) <=> epe m > 3 && epe m / max(sqrtf(gu^2 + gv^2), 1e-10) > 0.05    (float, as numpy's float32)
 *   errors[b, 0..7] = { epe, epe_noc, epe_occ, fl, epe_move, epe_static, fl_move, fl_static }
 *   counts[b, 0..4] = { S valid, S noc, S (valid - noc), S valid move, S valid (1 - move) }
 *     gt_channels == 2: epe = S epe / (H W), counts[b,0] = H W; every other column is NaN.
 *     gt_channels == 4: epe = S epe valid / S valid, epe_noc = S epe noc / S noc,
 *                       epe_occ = S epe (valid - noc) / max(S (valid - noc), 1), fl = 100 #bad(valid) / S valid;
 *     with move_mask:   epe_move = S epe valid move / S valid move, epe_static = S epe valid (1 - move) / S valid (1 - move),
 *                       fl_move = 100 #bad(valid move) / S valid move, fl_static = 100 #bad(valid (1 - move)) / S valid (1 - move);
 *                       without it columns 4..7 of errors and 3..4 of counts are NaN.
 *     A mean or rate whose denominator is 0 is NaN (numpy divides by zero there); epe_occ of such an item is 0.
 *   flow_up   [B,2,H,W] or NULL: receives (up, vp), the rescaled, resized flow, from the same pass; asking for it changes no bit
 *             of errors or counts.  With h == H and w == W it holds the bits of numpy's float32 pred / w * W.
 *   The per-pixel terms are fp32, their sums fp64; reproducible bit for bit: one record per workgroup of 256 pixels in the
 *   workspace, added in a fixed order by a second launch -- no atomics.  16-byte loads of the truth where H W is a multiple of 4
 *   and gt and move_mask are 16-byte aligned, the same values otherwise.
 *   workspace: pdepth_flow_metrics_workspace_bytes(B, H, W) bytes (104 bytes per 256 pixels), 256-byte aligned; 0 for
 *   non-positive sizes.  H W and h w at most 2^30, B at most 65535; a null pointer, gt_channels other than 2 or 4, a move mask
 *   with 2 channels: PDEPTH_E_ARG; a missing, short or misaligned workspace: PDEPTH_E_WORKSPACE; all before any launch.
 *
 * pdepth_flow_resize_f32: the rescale and the resize alone, the same sampling: flow [B,2,h,w] -> out [B,2,H,W] (not in place).
 *   align_corners 0: the rule above (the bits of flow_up).  align_corners 1: sx = x (w - 1) / (W - 1), 0 when W == 1, rows
 *   alike: utils/flow_utils.py:50-58 resize_flow (F.interpolate(align_corners=True), then the division by w / W and h / H).
 */
size_t pdepth_flow_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pdepth_flow_metrics_f32(const float *gt, int32_t gt_channels, const float *pred, int32_t h, int32_t w, const float *move_mask,
                            int32_t B, int32_t H, int32_t W, float *errors, float *counts, float *flow_up, void *workspace,
                            size_t workspace_bytes, void *stream);
int pdepth_flow_resize_f32(const float *flow, int32_t B, int32_t h, int32_t w, int32_t H, int32_t W, int32_t align_corners,
                           float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDEPTH_H_ */
