/* mcnerf_fit.h - C ABI of libmcnfit.so, the FIT library beside libmcnerf.so (include/mcnerf.h), libmcnext.so (include/mcnerf_ext.h),
 * libmcnreg.so (include/mcnerf_reg.h), libmcngeo.so (include/mcnerf_geo.h), libmcnbox.so (include/mcnerf_box.h) and libmcnhit.so
 * (include/mcnerf_hit.h).
 *
 * Those six ABIs are frozen at their version and prototype count; the entry points that fit the scene box to the voxel sigma cache live
 * here, in a seventh library that is loaded on first use only (mc_nerf_amd/_fit.py): a run that never sets the feature's key never opens
 * it.  The conventions are mcnerf.h's: device pointers owned by the caller, `stream` a hipStream_t as void*, nothing synchronises or
 * allocates, 0 = OK / negative = error with a thread-local message (mcnerf_fit_last_error), fp32 in and out.  Function names are
 * mcnerf_fit_*, defines MCNERF_FIT_*: the binding parses this header with the parser of mcnerf.h.
 *
 * This version: the box of "ray_bounds" = "aabb" mode fitted on the device to the occupied cells of the sigma grid and handed to the
 * ray-depth kernel without reaching the host (sys_param key "ray_bounds_fit" = "voxel").
 *
 * THE RULE, for a grid vox [G,G,G] over the cube [bmin, bmin + G h]^3 (linear index (ix G + iy) G + iz, as the voxel cache's), a
 * threshold, a margin in cells and an OUTER box; every floating-point step is a separately rounded fp32 operation:
 *   a cell is OCCUPIED iff vox[cell] > thresh -- the voxel select's comparison: NaN and a value equal to thresh are not, +inf is
 *   (1) i0_k, i1_k = the smallest and the largest index of the occupied cells on axis k;
 *       cells [8] int32 = (i0x, i0y, i0z, i1x, i1y, i1z, status, 0).  No cell occupied: cells[0:6] = (G, G, G, -1, -1, -1), status = 0,
 *       and the box is the outer box
 *   (2) otherwise  j0_k = max(i0_k - margin, 0),  j1_k = min(i1_k + margin, G - 1),
 *       lo_k = bmin + ((float) j0_k * h),  hi_k = bmin + ((float) (j1_k + 1) * h)
 *   (3) lo_k = fmaxf(lo_k, outer_lo_k),  hi_k = fminf(hi_k, outer_hi_k);  if any axis fails lo_k < hi_k all six values are the outer box
 *       and status = 2, otherwise status = 1
 *   (4) box [6] fp32 = (xmin, ymin, zmin, xmax, ymax, zmax)
 * Integer minima and maxima commute: two runs give the same bits.
 */
#ifndef MCNERF_FIT_H
#define MCNERF_FIT_H
#include "mcnerf.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MCNERF_FIT_ABI_VERSION 1

int mcnerf_fit_abi_version(void);
const char* mcnerf_fit_last_error(void);

/* cells [8] int32 and box [6] fp32 (both on the device, both written whole: the entry point initialises cells itself) of the grid vox
 * [G,G,G] by the rule above; h is the cell edge, formed by the caller in fp32 as float(bmax - bmin) / float(G).  One pass over the grid
 * (wide loads, grid-stride; a wave's and then a workgroup's minima and maxima are formed on chip, at most six integer atomics per
 * workgroup reach cells), and steps (2) - (4) in a launch behind it.  Refused before any device work: a null vox, cells or box, G outside
 * [2, 1024], h not finite or not > 0, a NaN bmin or thresh, margin < 0, an outer box that mcnerf_box_ray_depths would refuse (a
 * non-finite value, a min not below its max). */
int mcnerf_fit_voxel_box(const float* vox, int G, float bmin, float h, float thresh, int margin,
                         float xmin, float ymin, float zmin, float xmax, float ymax, float zmax,
                         int32_t* cells, float* box, void* stream);

/* mcnerf_hit_ray_depths (include/mcnerf_hit.h) with the box read from the device: box [6] fp32 = (xmin, ymin, zmin, xmax, ymax, zmax),
 * what mcnerf_fit_voxel_box writes.  z_c, z_f, span and hit (which may be NULL here) are the bits of mcnerf_box_ray_depths /
 * mcnerf_hit_ray_depths called with those six values: the same per-ray device function under a kernel that loads the box first.  The
 * box's values are not checked (they are device data: mcnerf_fit_voxel_box writes finite values with every min below its max, and a
 * NaN box leaves every ray unclipped by the rule of include/mcnerf_box.h); the other refusals are mcnerf_hit_ray_depths', and with
 * N > 0 a null box.  N = 0: nothing is read or written. */
int mcnerf_fit_ray_depths(const float* rays_o, const float* rays_d, int N, const float* box, float z_near, float z_far,
                          const float* jitter, const float* zgrid_c, int Sc, const float* zgrid_f, int Sf,
                          float* z_c, float* z_f, float* span, int32_t* hit, void* stream);

#ifdef __cplusplus
}
#endif
#endif
