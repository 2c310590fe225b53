/* mcnerf_ext.h - C ABI of libmcnext.so, the EXTENSION library beside libmcnerf.so (include/mcnerf.h).
 *
 * The core ABI is frozen at its version and prototype count; an opt-in feature whose kernels are not part of it lives here, in a
 * library of its own that is loaded on first use only (mc_nerf_amd/_ext.py): a run that never sets such a feature's key never opens
 * this library.  The conventions are mcnerf.h's: device pointers owned by the caller, `stream` a hipStream_t as void*, nothing
 * synchronises or allocates, 0 = OK / negative = error with a thread-local message (mcnerf_ext_last_error), fp32 throughout.
 * Function names are mcnerf_ext_*, defines MCNERF_EXT_*: the binding parses this header with the parser of mcnerf.h.
 *
 * This version: alpha-mask supervision of the FRONT weight (sys_param key "mask_weight").
 *
 *   w_j   = the rgb composite's own weights of mcnerf_composite_fwd (same eps draw, same 1e-10, delta not scaled by |d|)
 *   fg[n] = sum_{j = 0}^{S-2} w_j
 *
 * The last sample of a ray has delta = 1e10 and takes whatever transmittance is left, so sum_j w_j is 1 on EVERY ray, empty ones
 * included; what a mask can supervise is the weight in front of that far-plane sample.
 *
 * Inputs and outputs are fp32; mcnerf_ext_front_weight, and mcnerf_ext_composite_bwd_front when it is given d_fg, form each sample's
 * alpha and the transmittance product in fp64 (the device's expf is biased near 1 and the bias adds up over a thousand thin samples:
 * mc_nerf_amd/csrc/mask.hip).  Their weights are mcnerf_composite_fwd's to <= 6e-7 at S <= 128 and <= 6e-6 at S >= 1024.
 */
#ifndef MCNERF_EXT_H
#define MCNERF_EXT_H
#include "mcnerf.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MCNERF_EXT_ABI_VERSION 1

int mcnerf_ext_abi_version(void);
const char* mcnerf_ext_last_error(void);

/* fg [N] of the rays whose samples sig_rgb [N,S,4] mcnerf_composite_fwd composites: zgrid / z_stride / jitter / eps exactly as there
 * (z_stride 0: the shared grid [S]; S: rows [N,S]; jitter [N] or NULL).  One wave per ray, no LDS.  N = 0: nothing is read or written. */
int mcnerf_ext_front_weight(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                            int N, int S, float* fg, void* stream);

/* mcnerf_composite_bwd with one more upstream gradient: d_sig_rgb [N,S,4] of  sum rgb * d_rgb  +  sum fg * d_fg,  i.e. the gradient
 * of the weight of sample j is  d_rgb . (c_j - white_back)  +  (j + 1 < S ? d_fg[n] : 0).  The d_rgb part has that entry point's
 * form (its arithmetic word for word when d_fg is NULL); the d_fg part is added to d alpha_j last, in the closed form
 * d fg / d alpha_j = (T_{S-1} - 1e-10 sum_{j<k<S-1} T_k) / u_j,  which does not cancel where the front is opaque.  Everything
 * else is that entry point's: S <= MCNERF_EXT_BWD_MAX_SAMPLES (4 waves x 5 floats per sample of LDS), gmax_bits (or NULL) the running
 * maximum of |d_sig_rgb| as float bits, zero or a previous maximum on entry.  d_fg [N] or NULL; with NULL the result and the gmax word
 * are the bits of mcnerf_composite_bwd. */
#define MCNERF_EXT_BWD_MAX_SAMPLES 2048
int mcnerf_ext_composite_bwd_front(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                                   const float* d_rgb, const float* d_fg, int N, int S, int white_back,
                                   float* d_sig_rgb, uint32_t* gmax_bits, void* stream);

/* alpha[i] = (float)p[3] / 255.0f of pixel pix[i] of camera seg_cam[k], k the segment of ray i; 1.0 for 3-channel images.
 * images [C, npix, channels] uint8, channels 3 | 4; the n rays are K segments of consecutive rays as in mcnerf_ray_batch_fwd (HOST
 * arrays that travel by value in the kernel arguments, K <= MCNERF_MULTICAM_MAXSEG, refused when not monotone from 0 to n or when a
 * camera is outside [0, C)).  A pixel id outside [0, npix) reads nothing and gives NaN.  n = 0: nothing is read or written. */
int mcnerf_ext_gather_alpha(const uint8_t* images, int C, long long npix, int channels,
                            MCNERF_HOST const int32_t* seg_cam, MCNERF_HOST const int32_t* seg_start, int K,
                            const int64_t* pix, int n, float* alpha, void* stream);

/* The mask term and both gradients in one launch:
 *   out[0] = weight * out[1],   out[1] = mean_i (fg_c[i] - alpha[i])^2 + mean_i (fg_f[i] - alpha[i])^2   (the second without fg_f: 0)
 *   d_fg_c[i] = (2 weight / n) (fg_c[i] - alpha[i]),  d_fg_f likewise (with fg_f)
 * out holds MCNERF_EXT_MASK_LOSS_OUT floats: [2] unused, [3] the arrival counter (ZERO on entry, zero again on exit), [4 ...] the
 * block partials.  A fixed grid of at most 128 blocks; the block that arrives last adds the partials in block order: no float atomic,
 * the value does not depend on the order the blocks ran in.  fg_f / d_fg_f may be NULL together.  n = 0: nothing is read or written. */
#define MCNERF_EXT_MASK_LOSS_OUT 132
int mcnerf_ext_mask_loss(const float* fg_c, const float* fg_f, const float* alpha, int n, float weight,
                         float* out, float* d_fg_c, float* d_fg_f, void* stream);

#ifdef __cplusplus
}
#endif
#endif
