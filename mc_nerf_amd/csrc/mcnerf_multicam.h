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
// The segment k of ray i, its camera and its first ray `lo`: the last segment that starts at or before i (empty segments are passed
// over; the host checked that start is monotone from 0 to n).  Every table word is a wave-uniform scalar load and the three results
// are carried through the scan: indexing the by-value table with a per-lane k afterwards can push it into scratch.
struct McnSegment { int k, cam, lo; };
__device__ __forceinline__ McnSegment mcn_segment_of_ray(const McnSegTable& t, int i) {
    int k = 0, cam = t.cam[0], lo = 0;
    for (int s = 1; s < t.K; ++s) {
        const int st = t.start[s];
        if (i >= st) { k = s; cam = t.cam[s]; lo = st; }
    }
    return {k, cam, lo};
}
inline int mcn_longest_segment(const McnSegTable& t) {
    int longest = 0;
    for (int k = 0; k < t.K; ++k) longest = t.start[k + 1] - t.start[k] > longest ? t.start[k + 1] - t.start[k] : longest;
    return longest;
}
// The grid of a backward over the table: blockIdx.y = segment, 256 threads grid-striding over the longest segment in at most 512
// blocks in x.  x = 0: every segment is empty, nothing to launch.
inline dim3 mcn_segment_grid(const McnSegTable& t) {
    const int gx = (mcn_longest_segment(t) + 255) / 256;
    return dim3(gx > 512 ? 512 : gx, t.K);
}
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
