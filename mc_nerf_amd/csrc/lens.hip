// The ray preamble of a train step with per-camera radial lens distortion (`lens_model` = "radial"): the entry points
// and launchers of the ray-batch kernels with the lens option of mcnerf_rays.h on, that is with the undistortion of mcnerf_lens.h (the
// model is stated there) between the lift through the inverse intrinsics and the rotation.  The reference has no lens model.
//   lens_ray_batch_fwd_kernel: the body of ray_batch_fwd_kernel (the drawn ids are mcnerf_ray_batch_fwd's).  At lens = 0 every
//                  output has its bits.
//   lens_ray_batch_bwd_kernel: the body of ray_batch_bwd_kernel with the camera's 21 + 2 floats staged in LDS and 23 accumulators.
// K = 1 is a one-segment table: the single-camera step uses these kernels too when the feature is on.
#include "mcnerf_rays.h"

__global__ __launch_bounds__(256) void lens_ray_batch_fwd_kernel(McnLensRayBatchArgs b, McnSegTable t) {
    mcn_ray_batch_fwd_body<true>(b.r, b.lens, t);
}
hipError_t mcn_launch_lens_ray_batch_fwd(const McnLensRayBatchArgs& a, const McnSegTable& t, hipStream_t st) {
    if (a.r.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lens_ray_batch_fwd_kernel, dim3((a.r.n + 255) / 256), dim3(256), 0, st, a, t);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void lens_ray_batch_bwd_kernel(McnLensRayBatchBwdArgs b, McnSegTable t) {
    mcn_ray_batch_bwd_body<true>(b.r, b.lens, b.d_lens, t);
}
hipError_t mcn_launch_lens_ray_batch_bwd(const McnLensRayBatchBwdArgs& a, const McnSegTable& t, hipStream_t st) {
    const dim3 grid = mcn_segment_grid(t);
    if (grid.x == 0) return hipSuccess;
    hipLaunchKernelGGL(lens_ray_batch_bwd_kernel, grid, dim3(256), 0, st, a, t);
    return hipGetLastError();
}
