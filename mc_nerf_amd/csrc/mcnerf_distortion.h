// Launcher interface of the distortion-loss kernels (distortion.hip) between the regulariser library's C ABI (reg_api.hip,
// include/mcnerf_reg.h) and its kernels.  A header of its own, as mcnerf_mask.h: nothing of the other two libraries includes it.
#pragma once
#include "mcnerf_common.h"

#define MCN_DIST_MOMENT_BYTES 16      // (W, M) of a ray: two doubles

struct McnDistortionFwdArgs {
    const float* sig_rgb;   // [N,S,4]
    const float* zgrid;     // [S] (z_stride 0) or [N,S] rows (z_stride S), non-decreasing
    const float* jitter;    // [N] or null
    const float* eps;       // [N,S]
    int N, S, z_stride;
    float z_near, z_scale;  // s = (z - z_near) * z_scale
    float* dist;            // [N]
    double* moments;        // [N,2] = (W, M)
};
hipError_t mcn_launch_distortion_fwd(const McnDistortionFwdArgs& a, hipStream_t st);

struct McnCompositeBwdWArgs {
    const float* sig_rgb;
    const float* zgrid;
    const float* jitter;
    const float* eps;
    const float* d_rgb;     // [N,3]
    const float* d_fg;      // [N] or null
    const float* d_dist;    // [N] or null (then `moments` is not read)
    const double* moments;  // [N,2] of mcn_launch_distortion_fwd on the same inputs
    float z_near, z_scale;
    int N, S, white_back;
    float* d_sig_rgb;       // [N,S,4]
    unsigned* gmax_bits;    // or null
    int z_stride;
};
hipError_t mcn_launch_composite_bwd_w(const McnCompositeBwdWArgs& a, hipStream_t st);
