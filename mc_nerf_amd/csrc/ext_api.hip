// C ABI of libmcnext.so (see include/mcnerf_ext.h): the extension library beside libmcnerf.so.  Thin argument checking + launcher
// calls, as api.hip: every kernel is enqueued on the caller's stream, nothing here synchronises or allocates, and every refusal
// comes ahead of any device work.
#include "../../include/mcnerf_ext.h"
#include "mcnerf_mask.h"
#include "mcnerf_composite.h"
#include "mcnerf_api.h"

// the limits the public headers state are the kernels' own
static_assert(MCNERF_MULTICAM_MAXSEG == MCN_MULTICAM_MAXSEG, "include/mcnerf.h: MCNERF_MULTICAM_MAXSEG");
static_assert(MCNERF_EXT_MASK_LOSS_OUT == 4 + MCN_MASK_LOSS_BLOCKS, "include/mcnerf_ext.h: MCNERF_EXT_MASK_LOSS_OUT");
static_assert(MCNERF_EXT_BWD_MAX_SAMPLES == MCN_COMPOSITE_BWD_MAX_SAMPLES, "include/mcnerf_ext.h: MCNERF_EXT_BWD_MAX_SAMPLES");

extern "C" {

int mcnerf_ext_abi_version(void) { return MCNERF_EXT_ABI_VERSION; }
const char* mcnerf_ext_last_error(void) { return g_err; }

int mcnerf_ext_front_weight(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                            int N, int S, float* fg, void* stream) {
    REQ(N >= 0 && S > 0, "mcnerf_ext_front_weight");
    REQ((long long)N * S < (1ll << 31), "mcnerf_ext_front_weight");
    if (N == 0) return 0;                 // no rays: nothing is read or written (the empty arrays of a caller may be null pointers)
    REQ(sig_rgb && zgrid && eps && fg, "mcnerf_ext_front_weight");
    REQ(z_ok(z_stride, S), "mcnerf_ext_front_weight");
    McnFrontWeightArgs a = {sig_rgb, zgrid, jitter, eps, N, S, z_stride, fg};
    return check("mcnerf_ext_front_weight", mcn_launch_front_weight(a, (hipStream_t)stream));
}

int mcnerf_ext_composite_bwd_front(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                                   const float* d_rgb, const float* d_fg, int N, int S, int white_back,
                                   float* d_sig_rgb, uint32_t* gmax_bits, void* stream) {
    REQ(N >= 0 && S > 0, "mcnerf_ext_composite_bwd_front");
    REQ(S <= MCN_COMPOSITE_BWD_MAX_SAMPLES, "mcnerf_ext_composite_bwd_front");
    REQ((long long)N * S < (1ll << 31), "mcnerf_ext_composite_bwd_front");
    if (N == 0) return 0;
    REQ(sig_rgb && zgrid && eps && d_rgb && d_sig_rgb, "mcnerf_ext_composite_bwd_front");
    REQ(z_ok(z_stride, S), "mcnerf_ext_composite_bwd_front");
    McnCompositeBwdFrontArgs a = {sig_rgb, zgrid, jitter, eps, d_rgb, d_fg, N, S, white_back, d_sig_rgb, gmax_bits, z_stride};
    return check("mcnerf_ext_composite_bwd_front", mcn_launch_composite_bwd_front(a, (hipStream_t)stream));
}

int mcnerf_ext_gather_alpha(const uint8_t* images, int C, long long npix, int channels,
                            const int32_t* seg_cam, const int32_t* seg_start, int K,
                            const int64_t* pix, int n, float* alpha, void* stream) {
    McnSegTable t;
    if (int rc = fill_segments("mcnerf_ext_gather_alpha", t, seg_cam, seg_start, K, C, n, MCN_ANY_SEG)) return rc;
    REQ(npix >= 1 && (channels == 3 || channels == 4), "mcnerf_ext_gather_alpha");
    if (n == 0) return 0;
    REQ(images && pix && alpha, "mcnerf_ext_gather_alpha");
    McnGatherAlphaArgs a = {images, npix, channels, (const long long*)pix, n, alpha};
    return check("mcnerf_ext_gather_alpha", mcn_launch_gather_alpha(a, t, (hipStream_t)stream));
}

int mcnerf_ext_mask_loss(const float* fg_c, const float* fg_f, const float* alpha, int n, float weight,
                         float* out, float* d_fg_c, float* d_fg_f, void* stream) {
    REQ(n >= 0, "mcnerf_ext_mask_loss");
    REQ(weight >= 0.f && weight <= 3.0e38f, "mcnerf_ext_mask_loss");
    if (n == 0) return 0;
    REQ(fg_c && alpha && out && d_fg_c, "mcnerf_ext_mask_loss");
    REQ((fg_f == nullptr) == (d_fg_f == nullptr), "mcnerf_ext_mask_loss");
    return check("mcnerf_ext_mask_loss", mcn_launch_mask_loss(fg_c, fg_f, alpha, n, weight, out, d_fg_c, d_fg_f, (hipStream_t)stream));
}

}  // extern "C"
