// Launcher interface of the alpha-mask kernels (mask.hip) between the extension library's C ABI (ext_api.hip, include/mcnerf_ext.h)
// and its kernels.  A header of its own: mcnerf_kernels.h is part of the digest that ties the recorded MLP-kernel traffic to the sources.
#pragma once
#include "mcnerf_common.h"
#include "mcnerf_multicam.h"

#define MCN_MASK_LOSS_BLOCKS 128      // (include/mcnerf_ext.h: MCNERF_EXT_MASK_LOSS_OUT = 4 + MCN_MASK_LOSS_BLOCKS floats of `out`)

struct McnFrontWeightArgs {
    const float* sig_rgb;   // [N,S,4]
    const float* zgrid;     // [S] (z_stride 0) or [N,S] rows (z_stride S)
    const float* jitter;    // [N] or null
    const float* eps;       // [N,S]
    int N, S, z_stride;
    float* fg;              // [N]
};
hipError_t mcn_launch_front_weight(const McnFrontWeightArgs& a, hipStream_t st);

struct McnCompositeBwdFrontArgs {
    const float* sig_rgb;
    const float* zgrid;
    const float* jitter;
    const float* eps;
    const float* d_rgb;     // [N,3]
    const float* d_fg;      // [N] or null
    int N, S, white_back;
    float* d_sig_rgb;       // [N,S,4]
    unsigned* gmax_bits;    // or null
    int z_stride;
};
hipError_t mcn_launch_composite_bwd_front(const McnCompositeBwdFrontArgs& a, hipStream_t st);

struct McnGatherAlphaArgs {
    const unsigned char* images;   // [C, npix, channels]
    long long npix;
    int channels;
    const long long* pix;          // [n]
    int n;
    float* alpha;                  // [n]
};
hipError_t mcn_launch_gather_alpha(const McnGatherAlphaArgs& a, const McnSegTable& t, hipStream_t st);

hipError_t mcn_launch_mask_loss(const float* fg_c, const float* fg_f, const float* alpha, int n, float weight,
                                float* out, float* d_fg_c, float* d_fg_f, hipStream_t st);
