// C ABI of libmcnreg.so (see include/mcnerf_reg.h): the regulariser library beside libmcnerf.so and libmcnext.so.  Thin argument
// checking + launcher calls, as api.hip / ext_api.hip: every kernel is enqueued on the caller's stream, nothing here synchronises or
// allocates, and every refusal comes ahead of any device work.
#include "../../include/mcnerf_reg.h"
#include "mcnerf_distortion.h"
#include "mcnerf_composite.h"
#include "mcnerf_api.h"

// the limits the public header states are the kernels' own
static_assert(MCNERF_REG_BWD_MAX_SAMPLES == MCN_COMPOSITE_BWD_MAX_SAMPLES, "include/mcnerf_reg.h: MCNERF_REG_BWD_MAX_SAMPLES");
static_assert(MCNERF_REG_MOMENT_BYTES == MCN_DIST_MOMENT_BYTES && MCN_DIST_MOMENT_BYTES == 2 * sizeof(double), "include/mcnerf_reg.h: MCNERF_REG_MOMENT_BYTES");

extern "C" {

int mcnerf_reg_abi_version(void) { return MCNERF_REG_ABI_VERSION; }
const char* mcnerf_reg_last_error(void) { return g_err; }

int mcnerf_reg_distortion_fwd(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                              int N, int S, float z_near, float z_scale, float* dist, void* moments, void* stream) {
    REQ(N >= 0 && S > 0, "mcnerf_reg_distortion_fwd");
    REQ((long long)N * S < (1ll << 31), "mcnerf_reg_distortion_fwd");
    REQ(finite_f(z_near) && finite_f(z_scale), "mcnerf_reg_distortion_fwd");
    if (N == 0) return 0;                 // no rays: nothing is read or written (the empty arrays of a caller may be null pointers)
    REQ(sig_rgb && zgrid && eps && dist && moments, "mcnerf_reg_distortion_fwd");
    REQ(z_ok(z_stride, S), "mcnerf_reg_distortion_fwd");
    McnDistortionFwdArgs a = {sig_rgb, zgrid, jitter, eps, N, S, z_stride, z_near, z_scale, dist, (double*)moments};
    return check("mcnerf_reg_distortion_fwd", mcn_launch_distortion_fwd(a, (hipStream_t)stream));
}

int mcnerf_reg_composite_bwd_w(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                               const float* d_rgb, const float* d_fg, const float* d_dist, const void* moments,
                               float z_near, float z_scale, int N, int S, int white_back,
                               float* d_sig_rgb, uint32_t* gmax_bits, void* stream) {
    REQ(N >= 0 && S > 0, "mcnerf_reg_composite_bwd_w");
    REQ(S <= MCN_COMPOSITE_BWD_MAX_SAMPLES, "mcnerf_reg_composite_bwd_w");
    REQ((long long)N * S < (1ll << 31), "mcnerf_reg_composite_bwd_w");
    REQ(finite_f(z_near) && finite_f(z_scale), "mcnerf_reg_composite_bwd_w");
    REQ((d_dist == nullptr) == (moments == nullptr), "mcnerf_reg_composite_bwd_w");
    if (N == 0) return 0;
    REQ(sig_rgb && zgrid && eps && d_rgb && d_sig_rgb, "mcnerf_reg_composite_bwd_w");
    REQ(z_ok(z_stride, S), "mcnerf_reg_composite_bwd_w");
    McnCompositeBwdWArgs a = {sig_rgb, zgrid, jitter, eps, d_rgb, d_fg, d_dist, (const double*)moments, z_near, z_scale,
                              N, S, white_back, d_sig_rgb, gmax_bits, z_stride};
    return check("mcnerf_reg_composite_bwd_w", mcn_launch_composite_bwd_w(a, (hipStream_t)stream));
}

}  // extern "C"
