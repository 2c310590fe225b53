// C ABI of libmcnhit.so (see include/mcnerf_hit.h): the hit library beside libmcnerf.so, libmcnext.so, libmcnreg.so, libmcngeo.so and
// libmcnbox.so.  Thin argument checking + launcher calls, as api.hip / ext_api.hip / reg_api.hip / geo_api.hip / box_api.hip: every kernel
// is enqueued on the caller's stream, nothing here synchronises or allocates, and every refusal comes ahead of any device work.
#include "../../include/mcnerf_hit.h"
#include "mcnerf_ray_skip.h"
#include "mcnerf_api.h"

// what mcnerf_box_ray_depths takes: every finite float up to FLT_MAX (box_api.hip)
static bool box_finite(float v) { return v == v && v >= -3.4028235e38f && v <= 3.4028235e38f; }
// the voxel grid's geometry, as api.hip: 2 <= G <= 1024 cells per axis, a finite positive cells-per-unit scale
static bool vox_ok(int G, float bmin, float s) { return G >= 2 && G <= MCNERF_VOXEL_MAX_G && bmin == bmin && s > 0.f && s <= 3.0e38f; }

extern "C" {

int mcnerf_hit_abi_version(void) { return MCNERF_HIT_ABI_VERSION; }
const char* mcnerf_hit_last_error(void) { return g_err; }

int mcnerf_hit_ray_depths(const float* rays_o, const float* rays_d, int N,
                          float xmin, float ymin, float zmin, float xmax, float ymax, float zmax, float z_near, float z_far,
                          const float* jitter, const float* zgrid_c, int Sc, const float* zgrid_f, int Sf,
                          float* z_c, float* z_f, float* span, int32_t* hit, void* stream) {
    REQ(N >= 0 && Sc >= 1 && Sf >= 0, "mcnerf_hit_ray_depths");
    REQ((long long)N * (Sc > Sf ? Sc : Sf) < (1ll << 31), "mcnerf_hit_ray_depths");
    REQ(box_finite(xmin) && box_finite(ymin) && box_finite(zmin) && box_finite(xmax) && box_finite(ymax) && box_finite(zmax), "mcnerf_hit_ray_depths");
    REQ(xmin < xmax && ymin < ymax && zmin < zmax, "mcnerf_hit_ray_depths");
    REQ(box_finite(z_near) && box_finite(z_far) && z_far > z_near, "mcnerf_hit_ray_depths");
    if (N == 0) return 0;                 // no rays: nothing is read or written (the empty arrays of a caller may be null pointers)
    REQ(rays_o && rays_d && zgrid_c && z_c && hit, "mcnerf_hit_ray_depths");
    REQ((zgrid_f != nullptr) == (Sf > 0) && (z_f != nullptr) == (Sf > 0), "mcnerf_hit_ray_depths");
    McnRayDepthsArgs a = {rays_o, rays_d, N, {xmin, ymin, zmin}, {xmax, ymax, zmax}, z_near, z_far, jitter, zgrid_c, Sc, zgrid_f, Sf, z_c, z_f, span, hit};
    return check("mcnerf_hit_ray_depths", mcn_launch_ray_depths(a, (hipStream_t)stream));
}

int mcnerf_hit_list_rays(const int32_t* hit, int N, int S, float sigma_default, int32_t* ray_counts, int32_t* ray_offsets,
                         int32_t* idx, int32_t* count, float* out, void* stream) {
    REQ(N >= 0 && S >= 1, "mcnerf_hit_list_rays");
    REQ((long long)N * S < (1ll << 31), "mcnerf_hit_list_rays");
    if (N == 0) return 0;
    REQ(hit && ray_counts && ray_offsets && idx && count, "mcnerf_hit_list_rays");
    McnListRaysArgs a = {hit, N, S, 1, sigma_default, ray_counts, ray_offsets, (int2*)idx, count, out};
    return check("mcnerf_hit_list_rays", mcn_launch_list_rays(a, (hipStream_t)stream));
}

int mcnerf_hit_select_fine(const float* w_sel, const uint32_t* wmax_bits, float thresh, int N, int Sc, int scale,
                           float sigma_default, int32_t* ray_counts, int32_t* ray_offsets,
                           int32_t* idx, int32_t* count, float* out_f, const int32_t* hit, void* stream) {
    REQ(N >= 0 && Sc > 0 && scale > 0, "mcnerf_hit_select_fine");
    REQ((long long)N * Sc * scale < (1ll << 31), "mcnerf_hit_select_fine");
    if (N == 0) return 0;
    REQ(w_sel && wmax_bits && ray_counts && ray_offsets && idx && count && hit, "mcnerf_hit_select_fine");
    McnHitSelectArgs a = {{w_sel, wmax_bits, thresh, N, Sc, scale, sigma_default, ray_counts, ray_offsets, (int2*)idx, count, out_f}, hit};
    return check("mcnerf_hit_select_fine", mcn_launch_hit_select(a, (hipStream_t)stream));
}

int mcnerf_hit_voxel_select_rows(const float* vox, int G, float bmin, float s, float thresh, const float* rays_o, const float* rays_d,
                                 const float* z_rows, int N, int Sc, float sigma_default, int32_t* ray_counts,
                                 int32_t* ray_offsets, int32_t* idx, int32_t* count, float* out_c, const int32_t* hit, void* stream) {
    REQ(vox_ok(G, bmin, s) && N >= 0 && Sc > 0, "mcnerf_hit_voxel_select_rows");
    REQ((long long)N * Sc < (1ll << 31), "mcnerf_hit_voxel_select_rows");
    if (N == 0) return 0;
    REQ(vox && rays_o && rays_d && z_rows && ray_counts && ray_offsets && idx && count && hit, "mcnerf_hit_voxel_select_rows");
    McnHitVoxelSelectArgs a = {{vox, G, bmin, s, thresh, rays_o, rays_d, z_rows, nullptr, N, Sc, sigma_default, ray_counts, ray_offsets, (int2*)idx, count, out_c, Sc}, hit};
    return check("mcnerf_hit_voxel_select_rows", mcn_launch_hit_voxel_select(a, (hipStream_t)stream));
}

}  // extern "C"
