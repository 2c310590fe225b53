/* mcnerf_hit.h - C ABI of libmcnhit.so, the HIT library beside libmcnerf.so (include/mcnerf.h), libmcnext.so (include/mcnerf_ext.h),
 * libmcnreg.so (include/mcnerf_reg.h), libmcngeo.so (include/mcnerf_geo.h) and libmcnbox.so (include/mcnerf_box.h).
 *
 * Those five ABIs are frozen at their version and prototype count; the entry points that skip the rays missing the scene box live
 * here, in a sixth library that is loaded on first use only (mc_nerf_amd/_hit.py): a run that never sets the feature's key never opens
 * it.  The conventions are mcnerf.h's: device pointers owned by the caller, `stream` a hipStream_t as void*, nothing synchronises or
 * allocates, 0 = OK / negative = error with a thread-local message (mcnerf_hit_last_error), fp32 in and out.  Function names are
 * mcnerf_hit_*, defines MCNERF_HIT_*: the binding parses this header with the parser of mcnerf.h.
 *
 * This version: no sample of a ray that misses the box is listed for either net (sys_param key "ray_bounds_miss" = "skip", read in
 * "ray_bounds" = "aabb" mode).
 *
 * THE FLAG: hit[n] = 1 iff ray n is CLIPPED by the rule of include/mcnerf_box.h, else 0 -- a miss, a NaN or inf ray and a box that the
 * ray only grazes have hit = 0; a ray inside the box over all of [near, far] has hit = 1 with the span (near, far), so the span cannot
 * stand in for the flag.  Every list below names samples of rays with hit[n] != 0 only, in torch.nonzero (row-major) order, and no
 * wavefront of a ray with hit[n] == 0 reads that ray's weights or the sigma grid.  No atomic decides a position: two runs give the
 * same list.  ray_counts / ray_offsets are int32 [N] workspaces, idx takes int32 (ray, sample) pairs, *count their number (0 is legal
 * and leaves idx untouched); the prefilled output (or NULL) receives (sigma_default, 1, 1, 1) at every sample of EVERY ray.
 */
#ifndef MCNERF_HIT_H
#define MCNERF_HIT_H
#include "mcnerf.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MCNERF_HIT_ABI_VERSION 1

int mcnerf_hit_abi_version(void);
const char* mcnerf_hit_last_error(void);

/* mcnerf_box_ray_depths (include/mcnerf_box.h) with the flag: z_c, z_f and span are that entry point's bits, hit [N] (required) comes
 * from the same evaluation of the rule, in the same single launch.  The same refusals; N = 0: nothing is read or written. */
int mcnerf_hit_ray_depths(const float* rays_o, const float* rays_d, int N,
                          float xmin, float ymin, float zmin, float xmax, float ymax, float zmax, float z_near, float z_far,
                          const float* jitter, const float* zgrid_c, int Sc, const float* zgrid_f, int Sf,
                          float* z_c, float* z_f, float* span, int32_t* hit, void* stream);

/* Every pair (n, j), j < S, of the rays with hit[n] != 0 into idx [N*S]; *count = S * (number of such rays); out [N,S,4] or NULL.
 * Refused before any device work: N < 0, S < 1, N * S >= 2^31; with N > 0 also a null hit, workspace, idx or count.  N = 0: nothing
 * is read or written. */
int mcnerf_hit_list_rays(const int32_t* hit, int N, int S, float sigma_default, int32_t* ray_counts, int32_t* ray_offsets,
                         int32_t* idx, int32_t* count, float* out, void* stream);

/* mcnerf_select_fine (include/mcnerf.h) behind the flag: coarse sample (n, j) contributes its `scale` fine samples iff
 * hit[n] != 0 && w_sel[n,j] >= min(thresh, *wmax_bits as a float); list order, `scale` and the prefill of out_f [N,Sc*scale,4] are
 * mcnerf_select_fine's, and with hit all ones so is every bit.  N = 0: nothing is read or written. */
int mcnerf_hit_select_fine(const float* w_sel, const uint32_t* wmax_bits, float thresh, int N, int Sc, int scale,
                           float sigma_default, int32_t* ray_counts, int32_t* ray_offsets,
                           int32_t* idx, int32_t* count, float* out_f, const int32_t* hit, void* stream);

/* mcnerf_box_voxel_select_rows (include/mcnerf_box.h) behind the flag: pair (n, j) is listed iff hit[n] != 0 && vox[cell] > thresh,
 * the cell of the sample at depth z_rows[n,j].  Everything else is that entry point's.  N = 0: nothing is read or written. */
int mcnerf_hit_voxel_select_rows(const float* vox, int G, float bmin, float s, float thresh, const float* rays_o, const float* rays_d,
                                 const float* z_rows, int N, int Sc, float sigma_default, int32_t* ray_counts,
                                 int32_t* ray_offsets, int32_t* idx, int32_t* count, float* out_c, const int32_t* hit, void* stream);

#ifdef __cplusplus
}
#endif
#endif
