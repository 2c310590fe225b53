// C ABI of libmcngeo.so (see include/mcnerf_geo.h): the geometry library beside libmcnerf.so, libmcnext.so and libmcnreg.so.  Thin
// argument checking + launcher calls, as api.hip / ext_api.hip / reg_api.hip: every kernel is enqueued on the caller's stream, nothing
// here synchronises or allocates, and every refusal comes ahead of any device work.
#include "../../include/mcnerf_geo.h"
#include "mcnerf_depth.h"
#include "mcnerf_composite.h"
#include "mcnerf_api.h"

// the limits the public headers state are the kernels' own
static_assert(MCNERF_MULTICAM_MAXSEG == MCN_MULTICAM_MAXSEG, "include/mcnerf.h: MCNERF_MULTICAM_MAXSEG");
static_assert(MCNERF_GEO_BWD_MAX_SAMPLES == MCN_COMPOSITE_BWD_MAX_SAMPLES, "include/mcnerf_geo.h: MCNERF_GEO_BWD_MAX_SAMPLES");
static_assert(MCNERF_GEO_DEPTH_LOSS_OUT == 4 + 2 * MCN_DEPTH_LOSS_BLOCKS, "include/mcnerf_geo.h: MCNERF_GEO_DEPTH_LOSS_OUT");

extern "C" {

int mcnerf_geo_abi_version(void) { return MCNERF_GEO_ABI_VERSION; }
const char* mcnerf_geo_last_error(void) { return g_err; }

int mcnerf_geo_depth_fwd(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                         int N, int S, float* zexp, void* stream) {
    REQ(N >= 0 && S > 0, "mcnerf_geo_depth_fwd");
    REQ((long long)N * S < (1ll << 31), "mcnerf_geo_depth_fwd");
    if (N == 0) return 0;                 // no rays: nothing is read or written (the empty arrays of a caller may be null pointers)
    REQ(sig_rgb && zgrid && eps && zexp, "mcnerf_geo_depth_fwd");
    REQ(z_ok(z_stride, S), "mcnerf_geo_depth_fwd");
    McnDepthFwdArgs a = {sig_rgb, zgrid, jitter, eps, N, S, z_stride, zexp};
    return check("mcnerf_geo_depth_fwd", mcn_launch_depth_fwd(a, (hipStream_t)stream));
}

int mcnerf_geo_composite_bwd_z(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                               const float* d_rgb, const float* d_fg, const float* d_dist, const void* moments, const float* d_zexp,
                               float z_near, float z_scale, int N, int S, int white_back,
                               float* d_sig_rgb, uint32_t* gmax_bits, void* stream) {
    REQ(N >= 0 && S > 0, "mcnerf_geo_composite_bwd_z");
    REQ(S <= MCN_COMPOSITE_BWD_MAX_SAMPLES, "mcnerf_geo_composite_bwd_z");
    REQ((long long)N * S < (1ll << 31), "mcnerf_geo_composite_bwd_z");
    REQ((d_dist == nullptr) == (moments == nullptr), "mcnerf_geo_composite_bwd_z");
    REQ(d_dist == nullptr || (finite_f(z_near) && finite_f(z_scale)), "mcnerf_geo_composite_bwd_z");
    if (N == 0) return 0;
    REQ(sig_rgb && zgrid && eps && d_rgb && d_sig_rgb, "mcnerf_geo_composite_bwd_z");
    REQ(z_ok(z_stride, S), "mcnerf_geo_composite_bwd_z");
    McnCompositeBwdZArgs a = {sig_rgb, zgrid, jitter, eps, d_rgb, d_fg, d_dist, (const double*)moments, d_zexp, z_near, z_scale,
                              N, S, white_back, d_sig_rgb, gmax_bits, z_stride};
    return check("mcnerf_geo_composite_bwd_z", mcn_launch_composite_bwd_z(a, (hipStream_t)stream));
}

int mcnerf_geo_gather_depth(const float* depth, int C, long long HW, const int32_t* seg_cam, const int32_t* seg_start, int K,
                            const int64_t* pix, int n, float* out, void* stream) {
    McnSegTable t;
    if (int rc = fill_segments("mcnerf_geo_gather_depth", t, seg_cam, seg_start, K, C, n, MCN_ANY_SEG)) return rc;
    REQ(HW >= 1, "mcnerf_geo_gather_depth");
    if (n == 0) return 0;
    REQ(depth && pix && out, "mcnerf_geo_gather_depth");
    McnGatherDepthArgs a = {depth, HW, (const long long*)pix, n, out};
    return check("mcnerf_geo_gather_depth", mcn_launch_gather_depth(a, t, (hipStream_t)stream));
}

int mcnerf_geo_depth_loss(const float* zexp_c, const float* zexp_f, const float* d_gt, int n, float z_near, float z_scale, float weight,
                          float* out, float* d_c, float* d_f, void* stream) {
    REQ(n >= 0, "mcnerf_geo_depth_loss");
    REQ(weight >= 0.f && weight <= 3.0e38f, "mcnerf_geo_depth_loss");
    REQ(finite_f(z_near) && finite_f(z_scale), "mcnerf_geo_depth_loss");
    if (n == 0) return 0;
    REQ(zexp_c && d_gt && out && d_c, "mcnerf_geo_depth_loss");
    REQ((zexp_f == nullptr) == (d_f == nullptr), "mcnerf_geo_depth_loss");
    McnDepthLossArgs a = {zexp_c, zexp_f, d_gt, n, z_scale, weight, out, d_c, d_f};
    return check("mcnerf_geo_depth_loss", mcn_launch_depth_loss(a, (hipStream_t)stream));
}

}  // extern "C"
