// Launcher interface of the depth-supervision kernels (depth.hip) between the geometry library's C ABI (geo_api.hip,
// include/mcnerf_geo.h) and its kernels.  A header of its own, as mcnerf_mask.h and mcnerf_distortion.h: nothing of the other three
// libraries includes it.
#pragma once
#include "mcnerf_common.h"
#include "mcnerf_multicam.h"

#define MCN_DEPTH_LOSS_BLOCKS 128     // (include/mcnerf_geo.h: MCNERF_GEO_DEPTH_LOSS_OUT = 4 + 2 * MCN_DEPTH_LOSS_BLOCKS words of `out`)

struct McnDepthFwdArgs {
    const float* sig_rgb;   // [N,S,4]
    const float* zgrid;     // [S] (z_stride 0) or [N,S] rows (z_stride S)
    const float* jitter;    // [N] or null
    const float* eps;       // [N,S]
    int N, S, z_stride;
    float* zexp;            // [N]
};
hipError_t mcn_launch_depth_fwd(const McnDepthFwdArgs& a, hipStream_t st);

struct McnCompositeBwdZArgs {
    const float* sig_rgb;
    const float* zgrid;
    const float* jitter;
    const float* eps;
    const float* d_rgb;     // [N,3]
    const float* d_fg;      // [N] or null
    const float* d_dist;    // [N] or null (then `moments` is not read)
    const double* moments;  // [N,2] of the regulariser library's distortion forward on the same inputs
    const float* d_zexp;    // [N] or null
    float z_near, z_scale;
    int N, S, white_back;
    float* d_sig_rgb;       // [N,S,4]
    unsigned* gmax_bits;    // or null
    int z_stride;
};
hipError_t mcn_launch_composite_bwd_z(const McnCompositeBwdZArgs& a, hipStream_t st);

struct McnGatherDepthArgs {
    const float* depth;     // [C, npix]
    long long npix;
    const long long* pix;   // [n]
    int n;
    float* out;             // [n]
};
hipError_t mcn_launch_gather_depth(const McnGatherDepthArgs& a, const McnSegTable& t, hipStream_t st);

struct McnDepthLossArgs {
    const float* zexp_c;    // [n]
    const float* zexp_f;    // [n] or null
    const float* d_gt;      // [n]; valid: finite and > 0
    int n;
    float z_scale, weight;
    float* out;             // MCNERF_GEO_DEPTH_LOSS_OUT words
    float* d_c;             // [n]
    float* d_f;             // [n] or null
};
hipError_t mcn_launch_depth_loss(const McnDepthLossArgs& a, hipStream_t st);
