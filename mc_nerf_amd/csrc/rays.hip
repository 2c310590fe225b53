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
// tests/test_ray_preamble_gpu.py holds all six kernels to recorded outputs.
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
    mcn_ray_of_pixel(P, K, a.pix[i], a.W, a.rays_d, a.rays_o, i);
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
        mcn_raygen_bwd_ray(P, K, a.pix, a.W, a.d_rays_d, a.d_rays_o, i, acc);
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
// One thread per ray i.  Its segment is found by a scan of the table: every table word is a wave-uniform scalar load and the ray
// keeps the last segment that starts at or before it (empty segments are passed over; the host checked that start is monotone from
// 0 to n).  The camera's 21 matrix floats are read per ray through the cache: a block may straddle segments, so they cannot be
// staged once per block as raygen_fwd_kernel does.
__global__ __launch_bounds__(256) void ray_batch_fwd_kernel(McnRayBatchArgs a, McnSegTable t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int k = 0, cam = t.cam[0], lo = 0;
    for (int s = 1; s < t.K; ++s) {
        const int st = t.start[s];
        if (i >= st) { k = s; cam = t.cam[s]; lo = st; }
    }
    const unsigned npix = (unsigned)a.H * (unsigned)a.W;
    // segment k's own permutation of [0, H W): key *seed + k * 0x9E3779B9 (mod 2^32), so segment 0 draws what sample_perm_kernel draws
    const long long pid = a.pix_in ? a.pix_in[i] : (long long)mcn_feistel_perm((unsigned)(i - lo), npix, a.seed, (unsigned)k * 0x9E3779B9u);
    a.pix_out[i] = pid;
    mcn_ray_of_pixel(a.pose + (size_t)cam * 12, a.kinv + (size_t)cam * 9, pid, a.W, a.rays_d, a.rays_o, i);
    if (a.images) mcn_gt_of_pixel(a.images + ((size_t)cam * npix + (size_t)pid) * a.channels, a.channels, a.gt, i);
}

hipError_t mcn_launch_ray_batch_fwd(const McnRayBatchArgs& a, const McnSegTable& t, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ray_batch_fwd_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a, t);
    return hipGetLastError();
}

// Backward: blockIdx.y = segment.  A block grid-strides over its OWN segment only, so all its rays share one camera: the matrices
// are staged in LDS and the 21 accumulators reduced as in raygen_bwd_kernel, then one atomic per block and value goes into that
// camera's rows of d_pose [C,3,4] / d_kinv [C,3,3] (a camera listed in two segments receives both; the caller zeroes the outputs).
__global__ __launch_bounds__(256) void ray_batch_bwd_kernel(McnRayBatchBwdArgs a, McnSegTable t) {
    __shared__ float P[12], K[9];
    __shared__ float red[4][24];
    const int seg = blockIdx.y, cam = t.cam[seg], lo = t.start[seg], hi = t.start[seg + 1];
    if (lo + (int)(blockIdx.x * blockDim.x) >= hi) return;          // (block-uniform: no ray of this segment for this block)
    if (threadIdx.x < 12) P[threadIdx.x] = a.pose[(size_t)cam * 12 + threadIdx.x];
    if (threadIdx.x < 9) K[threadIdx.x] = a.kinv[(size_t)cam * 9 + threadIdx.x];
    __syncthreads();
    float acc[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) acc[k] = 0.f;
    for (int i = lo + blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += gridDim.x * blockDim.x) {
        mcn_raygen_bwd_ray(P, K, a.pix, a.W, a.d_rays_d, a.d_rays_o, i, acc);
    }
    mcn_raygen_bwd_flush(acc, P, red, a.d_pose + (size_t)cam * 12, a.d_kinv + (size_t)cam * 9);
}

hipError_t mcn_launch_ray_batch_bwd(const McnRayBatchBwdArgs& a, const McnSegTable& t, hipStream_t st) {
    int longest = 0;
    for (int k = 0; k < t.K; ++k) longest = max(longest, t.start[k + 1] - t.start[k]);
    if (longest <= 0) return hipSuccess;
    int gx = (longest + 255) / 256;
    if (gx > 512) gx = 512;
    hipLaunchKernelGGL(ray_batch_bwd_kernel, dim3(gx, t.K), dim3(256), 0, st, a, t);
    return hipGetLastError();
}
