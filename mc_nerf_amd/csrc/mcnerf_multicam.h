// Launcher interface of the multi-camera ray preamble (rays.hip) between the C ABI (api.hip) and its kernels.  A header of its
// own: mcnerf_kernels.h is part of the digest that ties the recorded MLP-kernel traffic (profiles/pmc_traffic_*.json) to the sources.
#pragma once
#include "mcnerf_common.h"

#define MCN_MULTICAM_MAXSEG 64      // segments (cameras) of one step; the table below is < 1 KB of kernel arguments
// The segment table of a multi-camera ray batch, passed BY VALUE in the kernel arguments (as McnFloats16 of upload_f32_kernel: no
// host-device copy, nothing for the host to wait on): segment k = rays [start[k], start[k+1]) of camera cam[k].
struct McnSegTable {
    int K;
    int cam[MCN_MULTICAM_MAXSEG];
    int start[MCN_MULTICAM_MAXSEG + 1];
};
struct McnRayBatchArgs {
    const float* pose;        // [C,3,4] world->cam of all cameras
    const float* kinv;        // [C,3,3]
    const long long* pix_in;  // [n] injected pixel ids, or null = draw on the device
    const unsigned* seed;     // device word keying the draw (read when pix_in is null)
    const unsigned char* images;   // [C, H*W, channels] uint8, or null = no ground truth
    int channels;             // 3 | 4
    int n, H, W;
    long long* pix_out;       // [n]
    float* rays_d;            // [n,3]
    float* rays_o;            // [n,3]
    float* gt;                // [n,3] (with images)
};
hipError_t mcn_launch_ray_batch_fwd(const McnRayBatchArgs& a, const McnSegTable& t, hipStream_t st);
struct McnRayBatchBwdArgs {
    const float* pose;
    const float* kinv;
    const long long* pix;     // [n] the pixels of the forward
    int W;
    const float* d_rays_d;    // [n,3]
    const float* d_rays_o;    // [n,3]
    float* d_pose;            // [C,12] accumulated (atomics)
    float* d_kinv;            // [C,9]
};
hipError_t mcn_launch_ray_batch_bwd(const McnRayBatchBwdArgs& a, const McnSegTable& t, hipStream_t st);
