// The ray preamble of a train step: draw the pixels, generate their rays from a camera's world->cam pose and inverse intrinsics
// (forward and backward), gather the ground truth from the camera's resident uint8 image.  Replaces MC_Model.get_rays +
// generate_rand_rays and the ground-truth gather (model/mc_nerf.py:124-145, 213-256, 327-345, 379, 80) for the selected pixels only.
//   one camera:    sample_perm_kernel, raygen_fwd_kernel / raygen_bwd_kernel, gather_gt_kernel -- one launch each;
//   `cams_per_step` > 1: the batch is K segments of consecutive rays, segment k = n_k rays of camera cam_k, and
//                  ray_batch_fwd_kernel does the three forward steps for every segment in ONE launch, ray_batch_bwd_kernel the
//                  backward; the reference has no such step.  The segment table travels by value in the kernel arguments
//                  (McnSegTable): no host-device copy, no host synchronisation.
// The single- and the multi-camera kernels call the same per-ray device functions (mcnerf_rays.h), so the fused launch gives the
// bits of the three single-camera launches by construction; tests/test_multicam_gpu.py compares them with torch.equal, and
// tests/test_ray_preamble_gpu.py holds all six kernels to recorded outputs.  The ray-batch kernels' bodies are in that header as
// well, with the lens model as a compile-time option: here they are instantiated without it, in lens.hip with it.
#include "mcnerf_kernels.h"
#include "mcnerf_multicam.h"
#include "mcnerf_rays.h"

// ------------------------------------------------------------------ one camera
// The pixel subset of a train step: randperm(H * W)[:batch] (model/mc_nerf.py:329, a uniformly random ordered subset without
// replacement) as `batch` evaluations of the keyed permutation mcn_feistel_perm (the cycle-walked domain is < 4 n, so < 4 walks on
// average).  One 7 us kernel instead of the 22 kernels of a device randperm of 640 000 keys (radix sort + merges, 0.2 ms/step).
__global__ __launch_bounds__(256) void sample_perm_kernel(long long* out, unsigned n, int batch, const unsigned* seed) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    out[i] = (long long)mcn_feistel_perm((unsigned)i, n, seed, 0u);
}
hipError_t mcn_launch_sample_perm(long long* out, long long n, int batch, const unsigned* seed, hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    hipLaunchKernelGGL(sample_perm_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, out, (unsigned)n, batch, seed);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void raygen_fwd_kernel(McnRaygenArgs a) {
    __shared__ float P[12], K[9];
    if (threadIdx.x < 12) P[threadIdx.x] = a.pose[threadIdx.x];
    if (threadIdx.x < 9) K[threadIdx.x] = a.kinv[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    mcn_ray_of_pixel<false>(P, K, nullptr, a.pix[i], a.W, a.rays_d, a.rays_o, i);
}
hipError_t mcn_launch_raygen_fwd(const McnRaygenArgs& a, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(raygen_fwd_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

// Backward: accumulates d_pose[3][4] and d_kinv[3][3] over the n rays (block reduction + one atomic per block and value).
__global__ __launch_bounds__(256) void raygen_bwd_kernel(McnRaygenBwdArgs a) {
    __shared__ float P[12], K[9];
    __shared__ float red[4][24];
    if (threadIdx.x < 12) P[threadIdx.x] = a.pose[threadIdx.x];
    if (threadIdx.x < 9) K[threadIdx.x] = a.kinv[threadIdx.x];
    __syncthreads();
    float acc[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) acc[k] = 0.f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
        mcn_raygen_bwd_ray<false>(P, K, nullptr, a.pix, a.W, a.d_rays_d, a.d_rays_o, i, acc);
    }
    mcn_raygen_bwd_flush(acc, P, red, a.d_pose, a.d_kinv);
}
hipError_t mcn_launch_raygen_bwd(const McnRaygenBwdArgs& a, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    int grid = (a.n + 255) / 256;
    if (grid > 512) grid = 512;
    hipLaunchKernelGGL(raygen_bwd_kernel, dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

// Device-resident images: GT colour of the selected pixels of one camera straight from uint8 images kept in
// HBM.  Replaces the 7.7 MB/step H2D copy of a float image plus `gt_rgbs.reshape(-1,3)[rand_idx]` (model/mc_nerf.py:379, 80).
__global__ __launch_bounds__(256) void gather_gt_kernel(const unsigned char* __restrict__ img, int channels,
                                                        const long long* __restrict__ pix, int n, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mcn_gt_of_pixel(img + (size_t)pix[i] * channels, channels, out, i);
}
hipError_t mcn_launch_gather_gt(const unsigned char* img, int channels, const long long* pix, int n, float* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_gt_kernel, dim3((n + 255) / 256), dim3(256), 0, st, img, channels, pix, n, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ a batch that spans cameras
// The bodies are mcnerf_rays.h's, here without its lens option (lens.hip holds the entry points with it).
__global__ __launch_bounds__(256) void ray_batch_fwd_kernel(McnRayBatchArgs a, McnSegTable t) {
    mcn_ray_batch_fwd_body<false>(a, nullptr, t);
}
hipError_t mcn_launch_ray_batch_fwd(const McnRayBatchArgs& a, const McnSegTable& t, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ray_batch_fwd_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a, t);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void ray_batch_bwd_kernel(McnRayBatchBwdArgs a, McnSegTable t) {
    mcn_ray_batch_bwd_body<false>(a, nullptr, nullptr, t);
}
hipError_t mcn_launch_ray_batch_bwd(const McnRayBatchBwdArgs& a, const McnSegTable& t, hipStream_t st) {
    const dim3 grid = mcn_segment_grid(t);
    if (grid.x == 0) return hipSuccess;
    hipLaunchKernelGGL(ray_batch_bwd_kernel, grid, dim3(256), 0, st, a, t);
    return hipGetLastError();
}
