/* mcnerf_box.h - C ABI of libmcnbox.so, the BOUNDS library beside libmcnerf.so (include/mcnerf.h), libmcnext.so
 * (include/mcnerf_ext.h), libmcnreg.so (include/mcnerf_reg.h) and libmcngeo.so (include/mcnerf_geo.h).
 *
 * Those four ABIs are frozen at their version and prototype count; the entry points of per-ray sample bounds live here, in a fifth
 * library that is loaded on first use only (mc_nerf_amd/_box.py): a run that never sets the feature's key never opens it.  The
 * conventions are mcnerf.h's: device pointers owned by the caller, `stream` a hipStream_t as void*, nothing synchronises or allocates,
 * 0 = OK / negative = error with a thread-local message (mcnerf_box_last_error), fp32 in and out.  Function names are mcnerf_box_*,
 * defines MCNERF_BOX_*: the binding parses this header with the parser of mcnerf.h.
 *
 * This version: sample depths clipped to an axis-aligned scene box (sys_param key "ray_bounds" = "aabb").
 *
 * THE RULE, per ray n with origin o and direction d; every step is a separately rounded fp32 operation, nothing is contracted:
 *   per axis k with d_k != 0:   t0 = (min_k - o_k) / d_k,  t1 = (max_k - o_k) / d_k,  the axis interval is [fminf(t0,t1), fmaxf(t0,t1)];
 *                               a NaN t0 or t1 (a NaN input, inf - inf, inf / inf) makes the ray a miss
 *   per axis k with d_k == 0 (either sign):  unconstrained when min_k <= o_k <= max_k, else the ray is a miss
 *   t_in  = the largest lower end,  t_out = the smallest upper end  (-inf / +inf when no axis constrains)
 *   lo = fmaxf(near, t_in),  hi = fminf(far, t_out)
 *   the ray is CLIPPED iff it is no miss, lo and hi are finite and hi > lo; otherwise lo = near, hi = far (a miss, a NaN or inf ray, a
 *   box that the ray only grazes: such a ray is sampled as without the box)
 *   a = (hi - lo) / (far - near),  b = lo - a * near
 *   z[n,j] = ((a * g[j]) + b) + (a * jitter[n])           (the last term absent when jitter is NULL)
 * An unclipped ray has a = 1 and b = 0 exactly, and its row is fl(g[j] + jitter[n]): the bits every kernel of the core library forms
 * from the shared grid.  Rows are non-decreasing in j for a non-decreasing g whatever the inputs (every step is a monotone rounding).
 */
#ifndef MCNERF_BOX_H
#define MCNERF_BOX_H
#include "mcnerf.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MCNERF_BOX_ABI_VERSION 1

int mcnerf_box_abi_version(void);
const char* mcnerf_box_last_error(void);

/* z_c [N,Sc] from the grid zgrid_c [Sc], z_f [N,Sf] from zgrid_f [Sf] (both NULL and Sf = 0: no second grid) and span [N,2] = (lo, hi)
 * (or NULL) of the rays rays_o / rays_d [N,3] against the box (xmin, ymin, zmin, xmax, ymax, zmax), by the rule above; jitter [N] or
 * NULL.  One launch, one wave per ray; no atomics, no LDS, no data-dependent loop; two runs give the same bits.  N = 0: nothing is read
 * or written.  Refused before any device work: N < 0, Sc < 1, Sf < 0, N * max(Sc, Sf) >= 2^31, a non-finite box or one with a min not
 * below its max, near or far non-finite or far <= near; with N > 0 also a null required pointer and zgrid_f / z_f / Sf not all or none. */
int mcnerf_box_ray_depths(const float* rays_o, const float* rays_d, int N,
                          float xmin, float ymin, float zmin, float xmax, float ymax, float zmax, float z_near, float z_far,
                          const float* jitter, const float* zgrid_c, int Sc, const float* zgrid_f, int Sf,
                          float* z_c, float* z_f, float* span, void* stream);

/* mcnerf_sample_pdf with the coarse depths of ray n read from z_rows[n, :] ([N,Sc], no jitter): the same device code, contract,
 * bounds (Sc >= 3, I >= 1, Sc + I <= MCNERF_PDF_MAX_SAMPLES) and LDS sizing.  With z_rows[n,j] = fl(zgrid[j] + jitter[n]) the result
 * is mcnerf_sample_pdf's bit for bit. */
int mcnerf_box_sample_pdf_rows(const float* w, const float* z_rows, const float* u, int N, int Sc, int I, float* z_all, void* stream);

/* mcnerf_voxel_select / mcnerf_voxel_update with the depth of sample j of ray n read from z_rows[n,j] ([N,Sc], no jitter): the same
 * device code and, for everything else, the same contracts (list order, count, prefill, single-writer max blend, scratch all zero
 * before and after). */
int mcnerf_box_voxel_select_rows(const float* vox, int G, float bmin, float s, float thresh, const float* rays_o, const float* rays_d,
                                 const float* z_rows, int N, int Sc, float sigma_default, int32_t* ray_counts,
                                 int32_t* ray_offsets, int32_t* idx, int32_t* count, float* out_c, void* stream);
int mcnerf_box_voxel_update_rows(float* vox, uint32_t* scratch, int G, float bmin, float s, float beta, float one_minus_beta,
                                 const float* rays_o, const float* rays_d, const float* z_rows, int N, int Sc,
                                 const int32_t* idx, const int32_t* count, int max_rows, const float* sig_rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif
