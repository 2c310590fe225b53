// Launcher interface of the bounds library (ray_bounds.hip) between its C-ABI (box_api.hip) and its kernels.
#pragma once
#include "mcnerf_kernels.h"
#include "mcnerf_voxel.h"

// per-ray sample depths from the scene box (the rule: include/mcnerf_box.h)
struct McnRayDepthsArgs {
    const float* rays_o;      // [N,3]
    const float* rays_d;      // [N,3]
    int N;
    float bmin[3], bmax[3];
    float z_near, z_far;
    const float* jitter;      // [N] or null
    const float* zgrid_c;     // [Sc]
    int Sc;
    const float* zgrid_f;     // [Sf] or null
    int Sf;
    float* z_c;               // [N,Sc] out
    float* z_f;               // [N,Sf] out, or null
    float* span;              // [N,2] out (lo, hi), or null
    int* hit = nullptr;       // [N] out, 1 iff the ray is CLIPPED, or null (the hit library's entry point gives it: include/mcnerf_hit.h)
};
hipError_t mcn_launch_ray_depths(const McnRayDepthsArgs& a, hipStream_t st);
// the sampler on rows: a.zgrid is [N,Sc], z_stride = Sc.  (The voxel select / update on rows are mcnerf_voxel.h's launchers with
// z_stride = Sc in their arguments.)
hipError_t mcn_launch_sample_pdf_rows(const McnSamplePdfArgs& a, hipStream_t st);
