/* mcnerf_geo.h - C ABI of libmcngeo.so, the GEOMETRY library beside libmcnerf.so (include/mcnerf.h), libmcnext.so
 * (include/mcnerf_ext.h) and libmcnreg.so (include/mcnerf_reg.h).
 *
 * Those three ABIs are frozen at their version and prototype count; the entry points of an opt-in geometric supervision of the
 * training render live here, in a fourth library that is loaded on first use only (mc_nerf_amd/_geo.py): a run that never sets such a
 * feature's key never opens it.  The conventions are mcnerf.h's: device pointers owned by the caller, `stream` a hipStream_t as void*,
 * nothing synchronises or allocates, 0 = OK / negative = error with a thread-local message (mcnerf_geo_last_error), fp32 in and out.
 * Function names are mcnerf_geo_*, defines MCNERF_GEO_*: the binding parses this header with the parser of mcnerf.h.
 *
 * This version: depth supervision of the expected depth (sys_param key "depth_weight").
 *
 *   z_j     = fl32(zrow[j] + jitter[n])       the composite's own depths
 *   w_j     = the rgb composite's own weights of mcnerf_composite_fwd (same eps draw, same 1e-10, delta not scaled by |d|, 1e10 for
 *             the far sample)
 *   zexp[n] = sum_{j = 0}^{S-1} w_j z_j
 *
 * The far-plane sample takes part at its depth z_{S-1}: it holds the transmittance that is left.  This is NOT the `depth` output of
 * mcnerf_composite_fwd (noise-free, |d|-scaled: a second weight family), which stays as it is.  Depths are constants of the backward:
 * the gradient reaches sig_rgb through w only.  Per-sample alpha, the transmittance product and sum w z are fp64, rounded once.
 * A depth TARGET is ray distance in world units (distance from the camera centre along the unit ray: the renderer's own z); it is a
 * measurement iff it is finite and > 0.
 */
#ifndef MCNERF_GEO_H
#define MCNERF_GEO_H
#include "mcnerf.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MCNERF_GEO_ABI_VERSION 1

int mcnerf_geo_abi_version(void);
const char* mcnerf_geo_last_error(void);

/* zexp [N] of the rays whose samples sig_rgb [N,S,4] mcnerf_composite_fwd composites: zgrid / z_stride / jitter / eps exactly as there
 * (z_stride 0: the shared grid [S]; S: rows [N,S]; jitter [N] or NULL).  One wave per ray, no LDS, no atomics, no bound on S; two runs
 * give the same bits.  N = 0: nothing is read or written. */
int mcnerf_geo_depth_fwd(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                         int N, int S, float* zexp, void* stream);

/* mcnerf_composite_bwd with up to three more upstream gradients: d_sig_rgb [N,S,4] of
 *   sum rgb * d_rgb  +  sum fg * d_fg  +  sum dist * d_dist  +  sum zexp * d_zexp,
 * fg the front weight of mcnerf_ext_front_weight (d_fg [N] or NULL), dist the term of mcnerf_reg_distortion_fwd (d_dist [N] with its
 * `moments` on the same inputs, z_near and z_scale; both or neither), zexp the expected depth above (d_zexp [N] or NULL): the gradient
 * of the weight of sample j gains d_zexp[n] * z_j.  Everything else is mcnerf_reg_composite_bwd_w's: S <= MCNERF_GEO_BWD_MAX_SAMPLES
 * (4 waves x 5 floats per sample of LDS), gmax_bits (or NULL) the running maximum of |d_sig_rgb| as float bits, zero or a previous
 * maximum on entry.  With d_zexp NULL the result and the gmax word are the bits of mcnerf_reg_composite_bwd_w for the same arguments.
 * Refused before any device work, outputs untouched: a null required pointer, S over the bound, z_stride neither 0 nor S,
 * N * S >= 2^31, d_dist without moments (or moments without d_dist), a non-finite z_near or z_scale when d_dist is given. */
#define MCNERF_GEO_BWD_MAX_SAMPLES 2048
int mcnerf_geo_composite_bwd_z(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                               const float* d_rgb, const float* d_fg, const float* d_dist, const void* moments, const float* d_zexp,
                               float z_near, float z_scale, int N, int S, int white_back,
                               float* d_sig_rgb, uint32_t* gmax_bits, void* stream);

/* out[i] = the depth target of pixel pix[i] of camera seg_cam[k], k the segment of ray i, when it is finite and > 0, else 0.0f (no
 * measurement).  depth [C, HW] fp32; the n rays are K segments of consecutive rays as in mcnerf_ray_batch_fwd (HOST arrays that travel
 * by value in the kernel arguments, K <= MCNERF_MULTICAM_MAXSEG, refused when not monotone from 0 to n or when a camera is outside
 * [0, C)).  A pixel id outside [0, HW) reads nothing and gives 0.0f.  n = 0: nothing is read or written. */
int mcnerf_geo_gather_depth(const float* depth, int C, long long HW,
                            MCNERF_HOST const int32_t* seg_cam, MCNERF_HOST const int32_t* seg_start, int K,
                            const int64_t* pix, int n, float* out, void* stream);

/* The depth term and both gradients in two launches, over the VALID rays (d_gt[i] finite and > 0; n_valid of them):
 *   s(z) = (z - z_near) * z_scale                          (z_scale = 1 / (far - near); only differences of s enter)
 *   out[1] = m = (1 / max(n_valid, 1)) sum_valid [ (s(zexp_c[i]) - s(d_gt[i]))^2 + (s(zexp_f[i]) - s(d_gt[i]))^2 ]   (zexp_f NULL: 0)
 *   out[0] = weight * m,   out[2] = n_valid
 *   d_c[i] = (2 weight z_scale / n_valid) (s(zexp_c[i]) - s(d_gt[i])) on valid rays, exactly 0.0f on the others; d_f likewise
 * With n_valid = 0 the term and every gradient are exactly 0.  out holds MCNERF_GEO_DEPTH_LOSS_OUT 4-byte words: [3] the arrival
 * counter (ZERO on entry, zero again on exit), [4 ...] the block partials of the sum and of the count.  A fixed grid of at most 128
 * blocks; the block that arrives last adds the partials in block order: no float atomic, the value does not depend on the order the
 * blocks ran in.  zexp_f / d_f may be NULL together.  Refused: n < 0, a negative or non-finite weight, a non-finite z_near or z_scale.
 * n = 0: nothing is read or written. */
#define MCNERF_GEO_DEPTH_LOSS_OUT 260
int mcnerf_geo_depth_loss(const float* zexp_c, const float* zexp_f, const float* d_gt, int n, float z_near, float z_scale, float weight,
                          float* out, float* d_c, float* d_f, void* stream);

#ifdef __cplusplus
}
#endif
#endif
