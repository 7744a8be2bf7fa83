// The host side of flow_warp's backward (flow_warp.hip), for the entries of flow_warp.hip itself and for cost_volume.hip, whose
// second launch is this backward with the gradient of the warped image as grad_out: one scatter, written once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace pdepth {
namespace flow {

// what the warp entries ask of their sizes and of `pad` alike (PDEPTH_OK, or PDEPTH_E_ARG with the message set)
int check_flow_warp(const char* who, int32_t B, int32_t C, int32_t H, int32_t W, int32_t pad);

// grad_flow [B,2,H,W], per owner (gflow != NULL), and grad_x [B,C,H,W] by float atomics, zeroed on the stream first (gx != NULL)
hipError_t launch_warp_backward(const float* x, const float* flo, const float* gout, int B, int C, int H, int W, int pad, float* gx,
                                float* gflow, hipStream_t s);

// the workspace of the integer-sum scatter of grad_x, and the backward with it (checked by the caller; unused when gx == NULL)
size_t warp_backward_det_workspace_bytes(int B, int C, int H, int W);
hipError_t launch_warp_backward_det(const float* x, const float* flo, const float* gout, int B, int C, int H, int W, int pad, float* gx,
                                    float* gflow, void* workspace, hipStream_t s);

}  // namespace flow
}  // namespace pdepth
