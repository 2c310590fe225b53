// Launcher interface of the voxel sigma cache (voxel.hip) between the C-ABI (api.hip) and its kernels; kept in a header of its own so that
// mcnerf_kernels.h -- part of the source digest that ties the recorded MLP-kernel profiles to their sources -- does not change with it.
#pragma once
#include "mcnerf_kernels.h"

// ---- voxel sigma cache (voxel.hip): the grid is vox [G,G,G] over [bmin, bmin + G / s]^3, s = G / (bmax - bmin) formed on the host
struct McnVoxelSelectArgs {
    const float* vox;         // [G,G,G] running raw sigma
    int G;
    float bmin, s, thresh;    // a sample is listed when vox[cell] > thresh
    const float* rays_o;      // [N,3]
    const float* rays_d;      // [N,3]
    const float* zgrid;       // [Sc], or [N,Sc] with z_stride = Sc
    const float* jitter;      // [N] or null
    int N, Sc;
    float sigma_default;
    int* ray_counts;          // [N] workspace
    int* ray_offsets;         // [N] workspace
    int2* idx;                // [N*Sc] out, torch.nonzero order
    int* count;               // out (device)
    float* out_c;             // [N,Sc,4] prefilled with (sigma_default,1,1,1), or null
    int z_stride = 0;         // 0: zgrid is the shared grid [Sc]; Sc: zgrid holds one row of depths per ray, [N,Sc]
};
hipError_t mcn_launch_voxel_select(const McnVoxelSelectArgs& a, hipStream_t st);
struct McnVoxelUpdateArgs {
    float* vox;               // [G,G,G]
    unsigned int* scratch;    // [G,G,G], all zero before and after
    int G;
    float bmin, s, beta, one_minus_beta;
    const float* pts;         // [M,3] explicit points with sigma [M], or null = the samples of rays:
    const float* sigma;
    int M;
    const float* rays_o;      // [N,3]
    const float* rays_d;      // [N,3]
    const float* zgrid;       // [Sc], or [N,Sc] with z_stride = Sc
    const float* jitter;      // [N] or null
    int N, Sc;
    const int2* idx;          // [max_rows] (ray, sample) pairs with *count of them valid, or null = all N * Sc pairs
    const int* count;
    int max_rows;
    const float* sig_rgb;     // [N,Sc,4]: sigma of pair (n, j) at ((n * Sc) + j) * 4
    int z_stride = 0;         // as McnVoxelSelectArgs::z_stride
};
hipError_t mcn_launch_voxel_update(const McnVoxelUpdateArgs& a, hipStream_t st);
hipError_t mcn_launch_voxel_query(const float* vox, int G, float bmin, float s, const float* pts, int M, float* out, hipStream_t st);
