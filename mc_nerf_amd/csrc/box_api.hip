// C ABI of libmcnbox.so (see include/mcnerf_box.h): the bounds library beside libmcnerf.so, libmcnext.so, libmcnreg.so and libmcngeo.so.
// Thin argument checking + launcher calls, as api.hip / ext_api.hip / reg_api.hip / geo_api.hip: every kernel is enqueued on the caller's
// stream, nothing here synchronises or allocates, and every refusal comes ahead of any device work.
#include "../../include/mcnerf_box.h"
#include "mcnerf_ray_bounds.h"
#include "mcnerf_api.h"

// the limits the public headers state are the kernels' own
static_assert(MCNERF_PDF_MAX_SAMPLES == MCN_PDF_MAX_SAMPLES, "include/mcnerf.h: MCNERF_PDF_MAX_SAMPLES");

// not mcnerf_api.h's finite_f, which stops at 3.0e38f: this library takes every finite float up to FLT_MAX, and what it refuses is as frozen as its header
static bool box_finite(float v) { return v == v && v >= -3.4028235e38f && v <= 3.4028235e38f; }
// the voxel grid's geometry, as api.hip: 2 <= G <= 1024 cells per axis, a finite positive cells-per-unit scale
static bool vox_ok(int G, float bmin, float s) { return G >= 2 && G <= MCNERF_VOXEL_MAX_G && bmin == bmin && s > 0.f && s <= 3.0e38f; }

extern "C" {

int mcnerf_box_abi_version(void) { return MCNERF_BOX_ABI_VERSION; }
const char* mcnerf_box_last_error(void) { return g_err; }

int mcnerf_box_ray_depths(const float* rays_o, const float* rays_d, int N,
                          float xmin, float ymin, float zmin, float xmax, float ymax, float zmax, float z_near, float z_far,
                          const float* jitter, const float* zgrid_c, int Sc, const float* zgrid_f, int Sf,
                          float* z_c, float* z_f, float* span, void* stream) {
    REQ(N >= 0 && Sc >= 1 && Sf >= 0, "mcnerf_box_ray_depths");
    REQ((long long)N * (Sc > Sf ? Sc : Sf) < (1ll << 31), "mcnerf_box_ray_depths");
    REQ(box_finite(xmin) && box_finite(ymin) && box_finite(zmin) && box_finite(xmax) && box_finite(ymax) && box_finite(zmax), "mcnerf_box_ray_depths");
    REQ(xmin < xmax && ymin < ymax && zmin < zmax, "mcnerf_box_ray_depths");
    REQ(box_finite(z_near) && box_finite(z_far) && z_far > z_near, "mcnerf_box_ray_depths");
    if (N == 0) return 0;                 // no rays: nothing is read or written (the empty arrays of a caller may be null pointers)
    REQ(rays_o && rays_d && zgrid_c && z_c, "mcnerf_box_ray_depths");
    REQ((zgrid_f != nullptr) == (Sf > 0) && (z_f != nullptr) == (Sf > 0), "mcnerf_box_ray_depths");
    McnRayDepthsArgs a = {rays_o, rays_d, N, {xmin, ymin, zmin}, {xmax, ymax, zmax}, z_near, z_far, jitter, zgrid_c, Sc, zgrid_f, Sf, z_c, z_f, span};
    return check("mcnerf_box_ray_depths", mcn_launch_ray_depths(a, (hipStream_t)stream));
}

int mcnerf_box_sample_pdf_rows(const float* w, const float* z_rows, const float* u, int N, int Sc, int I, float* z_all, void* stream) {
    REQ(N >= 0 && Sc >= 3 && I >= 1 && Sc + I <= MCN_PDF_MAX_SAMPLES, "mcnerf_box_sample_pdf_rows");
    if (N == 0) return 0;                 // (as mcnerf_sample_pdf)
    REQ(w && z_rows && u && z_all, "mcnerf_box_sample_pdf_rows");
    REQ((long long)N * (Sc + I) < (1ll << 31), "mcnerf_box_sample_pdf_rows");
    McnSamplePdfArgs a = {w, z_rows, nullptr, u, N, Sc, I, z_all};
    return check("mcnerf_box_sample_pdf_rows", mcn_launch_sample_pdf_rows(a, (hipStream_t)stream));
}

int mcnerf_box_voxel_select_rows(const float* vox, int G, float bmin, float s, float thresh, const float* rays_o, const float* rays_d,
                                 const float* z_rows, int N, int Sc, float sigma_default, int32_t* ray_counts,
                                 int32_t* ray_offsets, int32_t* idx, int32_t* count, float* out_c, void* stream) {
    REQ(vox && vox_ok(G, bmin, s) && rays_o && rays_d && z_rows && ray_counts && ray_offsets && idx && count && N >= 0 && Sc > 0, "mcnerf_box_voxel_select_rows");
    REQ((long long)N * Sc < (1ll << 31), "mcnerf_box_voxel_select_rows");
    McnVoxelSelectArgs a = {vox, G, bmin, s, thresh, rays_o, rays_d, z_rows, nullptr, N, Sc, sigma_default, ray_counts, ray_offsets, (int2*)idx, count, out_c, Sc};
    return check("mcnerf_box_voxel_select_rows", mcn_launch_voxel_select(a, (hipStream_t)stream));
}

int mcnerf_box_voxel_update_rows(float* vox, uint32_t* scratch, int G, float bmin, float s, float beta, float one_minus_beta,
                                 const float* rays_o, const float* rays_d, const float* z_rows, int N, int Sc,
                                 const int32_t* idx, const int32_t* count, int max_rows, const float* sig_rgb, void* stream) {
    REQ(vox && scratch && vox_ok(G, bmin, s) && rays_o && rays_d && z_rows && sig_rgb && N >= 0 && Sc > 0, "mcnerf_box_voxel_update_rows");
    REQ((idx == nullptr) == (count == nullptr) && max_rows >= 0 && (long long)N * Sc < (1ll << 31), "mcnerf_box_voxel_update_rows");
    McnVoxelUpdateArgs a = {vox, scratch, G, bmin, s, beta, one_minus_beta, nullptr, nullptr, 0, rays_o, rays_d, z_rows, nullptr, N, Sc,
                            (const int2*)idx, count, max_rows, sig_rgb, Sc};
    return check("mcnerf_box_voxel_update_rows", mcn_launch_voxel_update(a, (hipStream_t)stream));
}

}  // extern "C"
