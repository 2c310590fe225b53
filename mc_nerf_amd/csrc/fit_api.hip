// C ABI of libmcnfit.so (see include/mcnerf_fit.h): the fit library beside libmcnerf.so, libmcnext.so, libmcnreg.so, libmcngeo.so,
// libmcnbox.so and libmcnhit.so.  Thin argument checking + launcher calls, as api.hip / ext_api.hip / reg_api.hip / geo_api.hip /
// box_api.hip / hit_api.hip: every kernel is enqueued on the caller's stream, nothing here synchronises or allocates, and every refusal
// comes ahead of any device work.
#include "../../include/mcnerf_fit.h"
#include "mcnerf_scene_fit.h"
#include "mcnerf_api.h"

// what mcnerf_box_ray_depths takes: every finite float up to FLT_MAX (box_api.hip)
static bool box_finite(float v) { return v == v && v >= -3.4028235e38f && v <= 3.4028235e38f; }

extern "C" {

int mcnerf_fit_abi_version(void) { return MCNERF_FIT_ABI_VERSION; }
const char* mcnerf_fit_last_error(void) { return g_err; }

int mcnerf_fit_voxel_box(const float* vox, int G, float bmin, float h, float thresh, int margin,
                         float xmin, float ymin, float zmin, float xmax, float ymax, float zmax,
                         int32_t* cells, float* box, void* stream) {
    REQ(vox && cells && box, "mcnerf_fit_voxel_box");
    REQ(G >= 2 && G <= MCNERF_VOXEL_MAX_G, "mcnerf_fit_voxel_box");
    REQ(box_finite(h) && h > 0.f, "mcnerf_fit_voxel_box");
    REQ(bmin == bmin && thresh == thresh && margin >= 0, "mcnerf_fit_voxel_box");
    REQ(box_finite(xmin) && box_finite(ymin) && box_finite(zmin) && box_finite(xmax) && box_finite(ymax) && box_finite(zmax), "mcnerf_fit_voxel_box");
    REQ(xmin < xmax && ymin < ymax && zmin < zmax, "mcnerf_fit_voxel_box");
    McnVoxelBoxArgs a = {vox, G, bmin, h, thresh, margin, {xmin, ymin, zmin, xmax, ymax, zmax}, cells, box};
    return check("mcnerf_fit_voxel_box", mcn_launch_voxel_box(a, (hipStream_t)stream));
}

int mcnerf_fit_ray_depths(const float* rays_o, const float* rays_d, int N, const float* box, float z_near, float z_far,
                          const float* jitter, const float* zgrid_c, int Sc, const float* zgrid_f, int Sf,
                          float* z_c, float* z_f, float* span, int32_t* hit, void* stream) {
    REQ(N >= 0 && Sc >= 1 && Sf >= 0, "mcnerf_fit_ray_depths");
    REQ((long long)N * (Sc > Sf ? Sc : Sf) < (1ll << 31), "mcnerf_fit_ray_depths");
    REQ(box_finite(z_near) && box_finite(z_far) && z_far > z_near, "mcnerf_fit_ray_depths");
    if (N == 0) return 0;                 // no rays: nothing is read or written (the empty arrays of a caller may be null pointers)
    REQ(rays_o && rays_d && box && zgrid_c && z_c, "mcnerf_fit_ray_depths");
    REQ((zgrid_f != nullptr) == (Sf > 0) && (z_f != nullptr) == (Sf > 0), "mcnerf_fit_ray_depths");
    // (bmin / bmax stay zero here: the kernel loads them from `box`)
    McnRayDepthsArgs a = {rays_o, rays_d, N, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, z_near, z_far, jitter, zgrid_c, Sc, zgrid_f, Sf, z_c, z_f, span, hit};
    return check("mcnerf_fit_ray_depths", mcn_launch_fit_ray_depths(a, box, (hipStream_t)stream));
}

}  // extern "C"
