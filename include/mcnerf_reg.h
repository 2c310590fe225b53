/* mcnerf_reg.h - C ABI of libmcnreg.so, the REGULARISER library beside libmcnerf.so (include/mcnerf.h) and libmcnext.so
 * (include/mcnerf_ext.h).
 *
 * Both of those ABIs are frozen at their version and prototype count; the entry points of an opt-in regulariser of the compositing
 * weights live here, in a third library that is loaded on first use only (mc_nerf_amd/_reg.py): a run that never sets such a
 * feature's key never opens it.  The conventions are mcnerf.h's: device pointers owned by the caller, `stream` a hipStream_t as void*,
 * nothing synchronises or allocates, 0 = OK / negative = error with a thread-local message (mcnerf_reg_last_error), fp32 in and out.
 * Function names are mcnerf_reg_*, defines MCNERF_REG_*: the binding parses this header with the parser of mcnerf.h.
 *
 * This version: the distortion loss of mip-NeRF 360 on one pass's compositing weights (sys_param key "dist_weight").
 *
 *   z_j  = fl32(zrow[j] + jitter[n])          the composite's own depths; the rows must be NON-DECREASING
 *   w_j  = the rgb composite's own weights of mcnerf_composite_fwd (same eps draw, same 1e-10, delta not scaled by |d|, 1e10 for
 *          the far sample)
 *   s_j  = (z_j - z_near) * z_scale           (z_scale = 1 / (far - near); only differences of s enter)
 *   dist = sum_i sum_j w_i w_j |s_i - s_j|  +  (1/3) sum_{j < S-1} w_j^2 (s_{j+1} - s_j)
 *
 * The far-plane sample takes part in the pair term at its depth and has NO interval term (its "interval" is the 1e10 sentinel).
 * Depths are constants of the backward: the gradient reaches sig_rgb through w only.  The kernels use the O(S) prefix-sum form,
 * which is the definition only on non-decreasing rows.  Per-sample alpha, the transmittance product and the running sums are fp64.
 */
#ifndef MCNERF_REG_H
#define MCNERF_REG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MCNERF_REG_ABI_VERSION 1

int mcnerf_reg_abi_version(void);
const char* mcnerf_reg_last_error(void);

/* dist [N] of the rays whose samples sig_rgb [N,S,4] mcnerf_composite_fwd composites: zgrid / z_stride / jitter / eps exactly as there
 * (z_stride 0: the shared grid [S]; S: rows [N,S]; jitter [N] or NULL).  `moments` is an opaque buffer of N * MCNERF_REG_MOMENT_BYTES
 * bytes (8-byte aligned) that mcnerf_reg_composite_bwd_w takes back: the ray's (sum w, sum w s) in fp64.  One wave per ray, no LDS, no
 * atomics, no bound on S; two runs give the same bits.  N = 0: nothing is read or written. */
#define MCNERF_REG_MOMENT_BYTES 16
int mcnerf_reg_distortion_fwd(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                              int N, int S, float z_near, float z_scale, float* dist, void* moments, void* stream);

/* mcnerf_composite_bwd with up to two more upstream gradients: d_sig_rgb [N,S,4] of
 *   sum rgb * d_rgb  +  sum fg * d_fg  +  sum dist * d_dist,
 * fg the front weight of mcnerf_ext_front_weight (d_fg [N] or NULL), dist the term above (d_dist [N] with the `moments` of
 * mcnerf_reg_distortion_fwd on the same inputs, z_near and z_scale; both or neither).  With d_dist the gradient of the weight of sample
 * j gains d_dist[n] * d dist / d w_j,
 *   d dist / d w_j = 2 [ s_j (2 A_j + w_j - W) + M - 2 B_j - w_j s_j ]  +  (2/3) w_j (s_{j+1} - s_j) [j < S-1],
 * A_j, B_j the exclusive prefix sums of w and w s, (W, M) the moments.  Everything else is that entry point's:
 * S <= MCNERF_REG_BWD_MAX_SAMPLES (4 waves x 5 floats per sample of LDS), gmax_bits (or NULL) the running maximum of |d_sig_rgb| as
 * float bits, zero or a previous maximum on entry.  With d_dist NULL the result and the gmax word are the bits of
 * mcnerf_ext_composite_bwd_front for the same d_fg; with both NULL they are the bits of mcnerf_composite_bwd.
 * Refused before any device work, outputs untouched: a null required pointer, S over the bound, z_stride neither 0 nor S,
 * N * S >= 2^31, d_dist without moments (or moments without d_dist), a non-finite z_near or z_scale. */
#define MCNERF_REG_BWD_MAX_SAMPLES 2048
int mcnerf_reg_composite_bwd_w(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                               const float* d_rgb, const float* d_fg, const float* d_dist, const void* moments,
                               float z_near, float z_scale, int N, int S, int white_back,
                               float* d_sig_rgb, uint32_t* gmax_bits, void* stream);

#ifdef __cplusplus
}
#endif
#endif
