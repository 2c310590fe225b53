// Launcher interface of the fit library (scene_fit.hip) between its C-ABI (fit_api.hip) and its kernels.  The depths from a box on the
// device take mcnerf_ray_bounds.h's arguments (their bmin / bmax are not read: the kernel loads them from `box`).
#pragma once
#include "mcnerf_ray_bounds.h"

// the scene box fitted to the occupied cells of the sigma grid (the rule: include/mcnerf_fit.h)
struct McnVoxelBoxArgs {
    const float* vox;         // [G,G,G]
    int G;
    float bmin, h, thresh;    // the cube's corner, the cell edge, occupied iff vox[cell] > thresh
    int margin;               // cells added on every side
    float outer[6];           // (xmin, ymin, zmin, xmax, ymax, zmax): the box without an occupied cell, and the clamp of a fitted one
    int* cells;               // [8] out: (i0x, i0y, i0z, i1x, i1y, i1z, status, 0)
    float* box;               // [6] out
};
hipError_t mcn_launch_voxel_box(const McnVoxelBoxArgs& a, hipStream_t st);
hipError_t mcn_launch_fit_ray_depths(const McnRayDepthsArgs& a, const float* box, hipStream_t st);
