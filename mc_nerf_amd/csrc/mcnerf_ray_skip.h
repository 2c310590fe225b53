// Launcher interface of the hit library (ray_skip.hip) between its C-ABI (hit_api.hip) and its kernels.  The depths with the flag
// are mcnerf_ray_bounds.h's launcher with McnRayDepthsArgs::hit given.
#pragma once
#include "mcnerf_ray_bounds.h"

// every (n, j), j < Sc, of the rays with hit[n] != 0 (the names are McnSelectArgs': select.hip's kernel pair runs on them)
struct McnListRaysArgs {
    const int* hit;           // [N]
    int N, Sc, scale;         // scale is 1
    float sigma_default;
    int* ray_counts;          // [N] workspace
    int* ray_offsets;         // [N] workspace
    int2* idx;                // [N*Sc] out, torch.nonzero order
    int* count;               // out (device)
    float* out_f;             // [N,Sc,4] prefilled with (sigma_default,1,1,1), or null
};
hipError_t mcn_launch_list_rays(const McnListRaysArgs& a, hipStream_t st);
// the fine selection and the voxel list on rows behind the flag: the arguments of the lists they gate, and hit [N]
struct McnHitSelectArgs : McnSelectArgs { const int* hit; };
hipError_t mcn_launch_hit_select(const McnHitSelectArgs& a, hipStream_t st);
struct McnHitVoxelSelectArgs : McnVoxelSelectArgs { const int* hit; };
hipError_t mcn_launch_hit_voxel_select(const McnHitVoxelSelectArgs& a, hipStream_t st);
