// C ABI of the hot path (include/pdepth.h): argument validation + kernel dispatch of the sweep, pack, reduce, expect, warp_feature,
// sample_coords, ufield and backward entries, and pdepth_last_error().  Every other op keeps its entries beside its kernels.
// No torch types, no allocation, no host synchronisation.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "capi_util.hpp"
#include "kernels.hpp"
#include "sweep_workspace.hpp"

namespace {

using namespace pdepth::capi;

thread_local char g_err[512] = "";

size_t workspace_bytes_of(const pdepth_sweep_desc* d) { return pdepth::sweep_workspace_bytes(d->B, d->V, d->C, d->H, d->W); }
// a sweep workspace: present, large enough, 256-byte aligned
int check_sweep_workspace(const char* who, const pdepth_sweep_desc* d, const void* workspace, size_t bytes) {
    return check_workspace(who, workspace, bytes, workspace_bytes_of(d),
                           "; query pdepth_sweep_workspace_bytes()");
}

}  // namespace

// where every fail() of capi_util.hpp ends: the message pdepth_last_error() returns on this thread
int pdepth::api_error(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

namespace {

// does ALGO_AUTO run on a packed copy of the source for this shape?
bool uses_packed_source(const pdepth_sweep_desc* d) {
    return d->algo != PDEPTH_ALGO_DIRECT && d->D <= pdepth::sweep_tiled_max_planes() && d->W <= 32767 && d->H <= 32767 &&
           (long long)((d->C + 3) / 4 + 2) * d->H * d->W * 16 < (1ll << 31);
}

// Which sweep kernel family -- and with it which staging layout of the source -- a descriptor selects.  A pure function of
// the descriptor: the packing entry points and the sweep that follows decide alike.
//   distance form (sweep_dist.hip; layout dist_layout.hpp): what AUTO runs for L2, D <= 128, C <= 72, V <= 8
bool uses_dist(const pdepth_sweep_desc* d) {
    if (!uses_packed_source(d) || d->metric != PDEPTH_METRIC_L2) return false;
    if (d->algo != PDEPTH_ALGO_DIST && d->algo != PDEPTH_ALGO_AUTO) return false;
    return pdepth::sweep_dist_supports(make_args(d));
}
//   LDS-tiled kernel (sweep_tiled.hip; channel-group-planar layout): every other shape that fits a packed layout (L1 has no
//   distance form; wider features; more planes), and TILED_1 / TILED_2 on request
//   gather kernel (sweep_direct.hip; no packed source): ALGO_DIRECT and the shapes beyond the packed layouts
int source_layout(const pdepth_sweep_desc* d) {
    if (!uses_packed_source(d)) return PDEPTH_LAYOUT_NONE;
    if (uses_dist(d)) return PDEPTH_LAYOUT_DIST16;
    return PDEPTH_LAYOUT_C4;
}

// packed_ready: src is NULL and the workspace already holds the packed source (pdepth_pack_source_f32)
int sweep_common(const pdepth_sweep_desc* d, const pdepth_camera* cam, const float* ref,
                 const float* src, const float* d_candi, float* cost, float* logp, float* depth,
                 void* workspace, size_t workspace_bytes, void* stream, const char* who, bool packed_ready = false) {
    if (int rc = check_desc(d, cam, who)) return rc;
    if (!ref || (!src && !packed_ready) || !d_candi) return fail(PDEPTH_E_ARG, "%s: null input pointer", who);
    if (packed_ready && !uses_packed_source(d))
        return fail(PDEPTH_E_ARG, "%s: this shape / algorithm does not run on a packed source (use pdepth_sweep_dpv_f32)", who);
    if (!cost && !logp && !depth) return fail(PDEPTH_E_ARG, "%s: no output requested", who);
    if (d->metric != PDEPTH_METRIC_L2 && d->metric != PDEPTH_METRIC_L1)
        return fail(PDEPTH_E_ARG, "%s: undefined metric for feature distance (%d)", who, d->metric);
    if (d->algo < PDEPTH_ALGO_AUTO || d->algo > PDEPTH_ALGO_DIST)
        return fail(PDEPTH_E_ARG, "%s: unknown algo %d", who, d->algo);
    if (d->algo == PDEPTH_ALGO_CELLS || d->algo == PDEPTH_ALGO_MFMA || d->algo == PDEPTH_ALGO_CORR)
        return fail(PDEPTH_E_ARG, "%s: PDEPTH_ALGO_CELLS / PDEPTH_ALGO_MFMA / PDEPTH_ALGO_CORR are retired (the values stay reserved)", who);
    if (d->algo == PDEPTH_ALGO_DIST && !uses_dist(d))
        return fail(PDEPTH_E_ARG, "%s: PDEPTH_ALGO_DIST needs the L2 metric, D <= 128, C <= 72 and at most 8 source views", who);
    if (d->algo == PDEPTH_ALGO_TILED_2 && d->D > 64)
        return fail(PDEPTH_E_ARG, "%s: PDEPTH_ALGO_TILED_2 needs D <= 64", who);
    if (d->algo >= PDEPTH_ALGO_TILED_1 && !uses_packed_source(d))
        return fail(PDEPTH_E_ARG, "%s: the selected implementation does not support this shape", who);
    if (!(d->sigma > 0.0f) && !(d->sigma < 0.0f))
        return fail(PDEPTH_E_ARG, "%s: sigma must be non-zero", who);
    if (d->D > pdepth::sweep_direct_max_planes(d->C))
        return fail(PDEPTH_E_ARG, "%s: D=%d exceeds the %d planes one launch supports at C=%d", who,
                    d->D, pdepth::sweep_direct_max_planes(d->C), d->C);
    pdepth::SweepArgs a = make_args(d, cam, ref, src, d_candi);
    a.cost_out = cost; a.logp_out = logp; a.depth_out = depth;
    // the tiled kernel addresses one view through a 32-bit buffer descriptor (C*H*W*4 bytes < 2^31)
    // (the tiled kernels also pack a footprint as two 16-bit coordinates)
    if (uses_packed_source(d)) {
        if (int rc = check_sweep_workspace(who, d, workspace, workspace_bytes)) return rc;
        if (d->algo == PDEPTH_ALGO_TILED_1)
            return launched(pdepth::launch_sweep_tiled_n1(a, workspace, (hipStream_t)stream, packed_ready), who);
        if (d->algo == PDEPTH_ALGO_TILED_2)
            return launched(pdepth::launch_sweep_tiled_n2(a, workspace, (hipStream_t)stream, packed_ready), who);
        if (uses_dist(d)) return launched(pdepth::launch_sweep_dist(a, workspace, (hipStream_t)stream, packed_ready), who);
        return launched(pdepth::launch_sweep_tiled(a, workspace, (hipStream_t)stream, packed_ready), who);
    }
    return launched(pdepth::launch_sweep_direct(a, (hipStream_t)stream), who);
}

}  // namespace

extern "C" {

int pdepth_abi_version(void) { return PDEPTH_ABI_VERSION; }
const char* pdepth_last_error(void) { return g_err; }

size_t pdepth_sweep_workspace_bytes(const pdepth_sweep_desc* desc) {
    if (!desc || desc->algo == PDEPTH_ALGO_DIRECT) return 0;
    if (desc->B <= 0 || desc->D <= 0 || desc->H <= 0 || desc->W <= 0) return 0;
    return workspace_bytes_of(desc);
}

int pdepth_sweep_source_layout(const pdepth_sweep_desc* desc) {
    if (!desc || !dims_positive(desc)) return PDEPTH_LAYOUT_NONE;
    return source_layout(desc);
}

int pdepth_sweep_centres_source(const pdepth_sweep_desc* desc) {
    const int l = pdepth_sweep_source_layout(desc);
    return l == PDEPTH_LAYOUT_DIST16 ? 1 : 0;
}

int pdepth_sweep_cost_f32(const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* ref,
                          const float* src, const float* d_candi, float* cost, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (!cost) return fail(PDEPTH_E_ARG, "pdepth_sweep_cost_f32: null output");
    return sweep_common(desc, cam, ref, src, d_candi, cost, nullptr, nullptr, workspace, workspace_bytes,
                        stream, "pdepth_sweep_cost_f32");
}

int pdepth_sweep_dpv_f32(const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* ref,
                         const float* src, const float* d_candi, float* cost, float* logp,
                         float* depth, void* workspace, size_t workspace_bytes, void* stream) {
    return sweep_common(desc, cam, ref, src, d_candi, cost, logp, depth, workspace, workspace_bytes, stream,
                        "pdepth_sweep_dpv_f32");
}

int pdepth_pack_source_f32(const pdepth_sweep_desc* desc, const float* src, void* workspace, size_t workspace_bytes,
                           void* stream) {
    const char* who = "pdepth_pack_source_f32";
    if (!desc || !src) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_desc_dims(who, desc)) return rc;
    if (desc->src_vstride < (long long)desc->C * desc->H * desc->W || desc->src_bstride < 0)
        return fail(PDEPTH_E_ARG, "%s: bad strides", who);
    if (!uses_packed_source(desc))
        return fail(PDEPTH_E_ARG, "%s: this shape / algorithm does not run on a packed source", who);
    if (int rc = check_sweep_workspace(who, desc, workspace, workspace_bytes)) return rc;
    const pdepth::SweepArgs a = make_args(desc, nullptr, nullptr, src);
    if (uses_dist(desc)) return launched(pdepth::launch_pack_dist(a, workspace, (hipStream_t)stream), who);
    return launched(pdepth::launch_pack_c4(a, workspace, (hipStream_t)stream), who);
}

int pdepth_pack_views_f32(const pdepth_sweep_desc* desc, const float* feat, const float* rgb, int32_t pool_rate, float* ref_out,
                          void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pdepth_pack_views_f32";
    if (!desc || !feat || !rgb || !ref_out) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!dims_positive(desc) || desc->C <= 3 || pool_rate < 1)
        return fail(PDEPTH_E_ARG, "%s: bad dimension (C must count the 3 pooled image channels)", who);
    if (!uses_packed_source(desc))
        return fail(PDEPTH_E_ARG, "%s: this shape / algorithm does not run on a packed source", who);
    if ((long long)desc->H * pool_rate * desc->W * pool_rate * 3 >= (1ll << 31))
        return fail(PDEPTH_E_ARG, "%s: image too large", who);
    if (int rc = check_sweep_workspace(who, desc, workspace, workspace_bytes)) return rc;
    const pdepth::SweepArgs a = make_args(desc);
    if (uses_dist(desc))
        return launched(pdepth::launch_pack_views_dist(a, feat, rgb, pool_rate, desc->H * pool_rate, desc->W * pool_rate, ref_out, workspace,
                                                       (hipStream_t)stream), who);
    return launched(pdepth::launch_pack_views(a, feat, rgb, pool_rate, desc->H * pool_rate, desc->W * pool_rate, ref_out, workspace,
                                              (hipStream_t)stream), who);
}

int pdepth_sweep_dpv_packed_f32(const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* ref,
                                const float* d_candi, float* cost, float* logp, float* depth, void* workspace,
                                size_t workspace_bytes, void* stream) {
    return sweep_common(desc, cam, ref, nullptr, d_candi, cost, logp, depth, workspace, workspace_bytes, stream,
                        "pdepth_sweep_dpv_packed_f32", true);
}

int pdepth_dpv_reduce_f32(const float* logits, const float* d_candi, int32_t B, int32_t D, int32_t H,
                          int32_t W, float* logp, float* depth, void* stream) {
    if (!logits || !d_candi) return fail(PDEPTH_E_ARG, "pdepth_dpv_reduce_f32: null input");
    if (!logp && !depth) return fail(PDEPTH_E_ARG, "pdepth_dpv_reduce_f32: no output requested");
    if (int rc = check_dims("pdepth_dpv_reduce_f32", B, D, H, W)) return rc;
    return launched(pdepth::launch_dpv_reduce(logits, d_candi, B, D, H, W, logp, depth,
                                              (hipStream_t)stream), "pdepth_dpv_reduce_f32");
}

int pdepth_dpv_reduce_ex_f32(const float* logits, const float* addend, const float* d_candi, int32_t B, int32_t D,
                             int32_t H, int32_t W, float* logp, float* prob, float* depth, float* variance,
                             float* logp_quarter, void* stream) {
    const char* who = "pdepth_dpv_reduce_ex_f32";
    if (!logits || !d_candi) return fail(PDEPTH_E_ARG, "%s: null input", who);
    if (!logp && !prob && !depth && !variance && !logp_quarter) return fail(PDEPTH_E_ARG, "%s: no output requested", who);
    if (int rc = check_dims(who, B, D, H, W)) return rc;
    if (logp_quarter && (H < 4 || W < 4)) return fail(PDEPTH_E_ARG, "%s: quarter output needs H, W >= 4", who);
    if (prob == logits || variance == logits || (addend && (logp == addend || prob == addend)))
        return fail(PDEPTH_E_ARG, "%s: only logp may alias logits", who);
    return launched(pdepth::launch_dpv_reduce_ex(logits, addend, d_candi, B, D, H, W, logp, prob, depth, variance,
                                                 logp_quarter, (hipStream_t)stream), who);
}

int pdepth_dpv_expect_f32(const float* dpv, const float* d_candi, int32_t B, int32_t D, int32_t H,
                          int32_t W, int32_t bv_log, float* depth, void* stream) {
    if (!dpv || !d_candi || !depth) return fail(PDEPTH_E_ARG, "pdepth_dpv_expect_f32: null pointer");
    if (int rc = check_dims("pdepth_dpv_expect_f32", B, D, H, W)) return rc;
    return launched(pdepth::launch_dpv_expect(dpv, d_candi, B, D, H, W, bv_log, depth,
                                              (hipStream_t)stream), "pdepth_dpv_expect_f32");
}

int pdepth_warp_feature_f32(const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* src,
                            const float* d_candi, float* out, void* stream) {
    if (int rc = check_desc(desc, cam, "pdepth_warp_feature_f32")) return rc;
    if (!src || !d_candi || !out) return fail(PDEPTH_E_ARG, "pdepth_warp_feature_f32: null pointer");
    if (desc->C != desc->D)
        return fail(PDEPTH_E_ARG, "pdepth_warp_feature_f32: needs C == D (got C=%d D=%d)", desc->C, desc->D);
    pdepth::SweepArgs a = make_args(desc, cam, nullptr, src, d_candi);
    return launched(pdepth::launch_warp_feature(a, out, (hipStream_t)stream), "pdepth_warp_feature_f32");
}

int pdepth_sample_coords_f32(const pdepth_sweep_desc* desc, const pdepth_camera* cam,
                             const float* d_candi, float* ix, float* iy, void* stream) {
    if (!desc || !cam) return fail(PDEPTH_E_ARG, "pdepth_sample_coords_f32: null descriptor");
    pdepth_sweep_desc d = *desc;
    if (d.C <= 0) d.C = 1;
    d.src_vstride = (long long)d.C * d.H * d.W;
    if (int rc = check_desc(&d, cam, "pdepth_sample_coords_f32")) return rc;
    if (!d_candi || !ix || !iy) return fail(PDEPTH_E_ARG, "pdepth_sample_coords_f32: null pointer");
    pdepth::SweepArgs a = make_args(&d, cam, nullptr, nullptr, d_candi);
    return launched(pdepth::launch_sample_coords(a, ix, iy, (hipStream_t)stream), "pdepth_sample_coords_f32");
}

size_t pdepth_ufield_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return (B > 0 && H > 0 && W > 0) ? pdepth::ufield_workspace_bytes(B, H, W) : 0;
}

int pdepth_ufield_f32(const float* dpv, const float* d_candi, const float* intr, const float* mask, int32_t B, int32_t D,
                      int32_t H, int32_t W, int32_t bv_log, float unc_ang, float z_start, float z_end, float min_depth,
                      int32_t quash, float oob_depth, float* plane, float* depth_zero, void* workspace,
                      size_t workspace_bytes, void* stream) {
    const char* who = "pdepth_ufield_f32";
    if (!dpv || !d_candi || !intr || !plane || !depth_zero) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return fail(PDEPTH_E_ARG, "%s: bad dimension", who);
    // the sampling grid of a shift divides by size - 1 (convert_flowfield): a single row or column can only be collapsed unshifted
    if (unc_ang != 0.0f && (H <= 1 || W <= 1)) return fail(PDEPTH_E_ARG, "%s: a shift needs H, W >= 2", who);
    const size_t need = pdepth::ufield_workspace_bytes(B, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(PDEPTH_E_WORKSPACE, "%s: needs %zu bytes of workspace (got %zu)", who, need, workspace_bytes);
    return launched(pdepth::launch_ufield(dpv, d_candi, intr, mask, B, D, H, W, bv_log, unc_ang, z_start, z_end, min_depth,
                                          quash, oob_depth, plane, depth_zero, workspace, (hipStream_t)stream), who);
}

// est_swp_volume_v4 backward (warping/homography.py:98-135, :170-198, :80-86), features only
int pdepth_sweep_backward_f32(const pdepth_sweep_desc* desc, const pdepth_camera* cam, const float* ref, const float* src,
                              const float* d_candi, const float* grad_cost, float* grad_ref, float* grad_src, void* stream) {
    const char* who = "pdepth_sweep_backward_f32";
    if (int rc = check_sweep_backward(who, desc, cam, ref, src, d_candi, grad_cost, grad_ref, grad_src)) return rc;
    pdepth::SweepArgs a = make_args(desc, cam, ref, src, d_candi);
    a.fast_div = 0;
    return launched(pdepth::launch_sweep_backward(a, grad_cost, grad_ref, grad_src, (hipStream_t)stream), who);
}

// F.log_softmax(dim=1) + exp + dpv_to_depthmap(BV_log=True) backward (models/models.py:694, :697; utils/img_utils.py:52-61)
int pdepth_dpv_reduce_backward_f32(const float* logp, const float* d_candi, int32_t B, int32_t D, int32_t H, int32_t W,
                                   const float* g_logp, const float* g_prob, const float* g_depth, float* g_logits, void* stream) {
    const char* who = "pdepth_dpv_reduce_backward_f32";
    if (!logp || !d_candi || !g_logits) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (!g_logp && !g_prob && !g_depth) return fail(PDEPTH_E_ARG, "%s: no incoming gradient", who);
    if (int rc = check_dims(who, B, D, H, W)) return rc;
    if ((long long)H * W > (1ll << 30)) return fail(PDEPTH_E_ARG, "%s: H*W too large", who);
    if ((const float*)g_logits == logp || (g_prob && (const float*)g_logits == g_prob))
        return fail(PDEPTH_E_ARG, "%s: only g_logp may alias g_logits", who);
    return launched(pdepth::launch_dpv_reduce_backward(logp, d_candi, B, D, H, W, g_logp, g_prob, g_depth, g_logits,
                                                       (hipStream_t)stream), who);
}

// dpv_to_depthmap backward (utils/img_utils.py:52-61)
int pdepth_dpv_expect_backward_f32(const float* dpv, const float* d_candi, int32_t B, int32_t D, int32_t H, int32_t W,
                                   int32_t bv_log, const float* g_depth, float* g_dpv, void* stream) {
    const char* who = "pdepth_dpv_expect_backward_f32";
    if (!dpv || !d_candi || !g_depth || !g_dpv) return fail(PDEPTH_E_ARG, "%s: null pointer", who);
    if (int rc = check_dims(who, B, D, H, W)) return rc;
    if ((long long)H * W > (1ll << 30)) return fail(PDEPTH_E_ARG, "%s: H*W too large", who);
    if ((const float*)g_dpv == dpv || (const float*)g_dpv == g_depth) return fail(PDEPTH_E_ARG, "%s: g_dpv may not alias an input", who);
    return launched(pdepth::launch_dpv_expect_backward(dpv, d_candi, B, D, H, W, bv_log, g_depth, g_dpv, (hipStream_t)stream), who);
}

}  // extern "C"
