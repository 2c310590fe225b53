// The ray preamble of a train step with per-camera radial lens distortion (`lens_model` = "radial"): the fused
// ray-batch kernels of rays.hip with the undistortion of mcnerf_lens.h (the model is stated there) between the lift through the
// inverse intrinsics and the rotation.  The reference has no lens model.
//   lens_ray_batch_fwd_kernel: one thread per ray, the segment found as ray_batch_fwd_kernel does, the pixel injected or drawn by
//                  mcn_feistel_perm under the same key rule (the drawn ids are mcnerf_ray_batch_fwd's), the ground truth through
//                  mcn_gt_of_pixel.  At lens = 0 every output has the bits of ray_batch_fwd_kernel.
//   lens_ray_batch_bwd_kernel: blockIdx.y = segment, the camera's 21 + 2 floats staged in LDS, 23 accumulators: the 21 of
//                  raygen_bwd reduced and flushed by mcn_raygen_bwd_flush, the two lens sums through the spare columns of the same
//                  LDS array; one float atomic per block and value.
// K = 1 is a one-segment table: the single-camera step uses these kernels too when the feature is on.
#include "mcnerf_lens.h"
#include "mcnerf_rays.h"

__global__ __launch_bounds__(256) void lens_ray_batch_fwd_kernel(McnLensRayBatchArgs b, McnSegTable t) {
    const McnRayBatchArgs& a = b.r;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int k = 0, cam = t.cam[0], lo = 0;
    for (int s = 1; s < t.K; ++s) {
        const int st = t.start[s];
        if (i >= st) { k = s; cam = t.cam[s]; lo = st; }
    }
    const unsigned npix = (unsigned)a.H * (unsigned)a.W;
    const long long pid = a.pix_in ? a.pix_in[i] : (long long)mcn_feistel_perm((unsigned)(i - lo), npix, a.seed, (unsigned)k * 0x9E3779B9u);
    a.pix_out[i] = pid;
    float c3[3], s, r;
    mcn_cam_of_pixel(a.kinv + (size_t)cam * 9, pid, a.W, c3);
    mcn_lens_undistort_cam(c3, b.lens[(size_t)cam * 2], b.lens[(size_t)cam * 2 + 1], &s, &r);
    mcn_ray_of_cam(a.pose + (size_t)cam * 12, c3, a.rays_d, a.rays_o, i);
    if (a.images) mcn_gt_of_pixel(a.images + ((size_t)cam * npix + (size_t)pid) * a.channels, a.channels, a.gt, i);
}

hipError_t mcn_launch_lens_ray_batch_fwd(const McnLensRayBatchArgs& a, const McnSegTable& t, hipStream_t st) {
    if (a.r.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lens_ray_batch_fwd_kernel, dim3((a.r.n + 255) / 256), dim3(256), 0, st, a, t);
    return hipGetLastError();
}

// One ray's 23 terms: acc[0..20] as mcn_raygen_bwd_ray (dR from the UNDISTORTED cam, dKinv from the gradient carried back through
// the undistortion), acc[21..22] d k1, d k2.  P, K, L: the camera's matrices and coefficients (LDS).
__device__ __forceinline__ void lens_raygen_bwd_ray(const float* P, const float* K, const float* L, const long long* pix, int W,
                                                    const float* d_rays_d, const float* d_rays_o, int i, float* acc) {
    const long long pid = pix[i];
    const float p[3] = {(float)(pid % W) + 0.5f, (float)(pid / W) + 0.5f, 1.f};
    float cam[3], gcam[3], ds[3], s, r;
#pragma unroll
    for (int j = 0; j < 3; ++j) cam[j] = p[0] * K[j * 3] + p[1] * K[j * 3 + 1] + K[j * 3 + 2];
    const float xd = cam[0], yd = cam[1];
    mcn_lens_undistort_cam(cam, L[0], L[1], &s, &r);
    mcn_raygen_bwd_cam(P, cam, d_rays_d, i, gcam, acc);
    mcn_lens_ds(s, r, L[0], L[1], ds);
    const float h = gcam[0] * xd + gcam[1] * yd;
    acc[21] += h * ds[0];
    acc[22] += h * ds[1];
    const float hx = h * ds[2];
    gcam[0] = gcam[0] * s + hx * xd;
    gcam[1] = gcam[1] * s + hx * yd;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[9 + j * 3 + k] += gcam[j] * p[k];     // dKinv[j][k]
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[18 + c] += d_rays_o[i * 3 + c];            // sum of origin gradients
}

__global__ __launch_bounds__(256) void lens_ray_batch_bwd_kernel(McnLensRayBatchBwdArgs b, McnSegTable t) {
    __shared__ float P[12], K[9], L[2];
    __shared__ float red[4][24];
    const McnRayBatchBwdArgs& a = b.r;
    const int seg = blockIdx.y, cam = t.cam[seg], lo = t.start[seg], hi = t.start[seg + 1];
    if (lo + (int)(blockIdx.x * blockDim.x) >= hi) return;          // (block-uniform: no ray of this segment for this block)
    if (threadIdx.x < 12) P[threadIdx.x] = a.pose[(size_t)cam * 12 + threadIdx.x];
    if (threadIdx.x < 9) K[threadIdx.x] = a.kinv[(size_t)cam * 9 + threadIdx.x];
    if (threadIdx.x < 2) L[threadIdx.x] = b.lens[(size_t)cam * 2 + threadIdx.x];
    __syncthreads();
    float acc[23];
#pragma unroll
    for (int k = 0; k < 23; ++k) acc[k] = 0.f;
    for (int i = lo + blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += gridDim.x * blockDim.x) {
        lens_raygen_bwd_ray(P, K, L, a.pix, a.W, a.d_rays_d, a.d_rays_o, i, acc);
    }
    // the two lens sums ride in columns 21, 22 of `red`, which mcn_raygen_bwd_flush leaves alone; its barrier orders them too
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 21; k < 23; ++k) {
        float v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wv][k] = v;
    }
    mcn_raygen_bwd_flush(acc, P, red, a.d_pose + (size_t)cam * 12, a.d_kinv + (size_t)cam * 9);
    if (threadIdx.x >= 21 && threadIdx.x < 23) {
        const int k = threadIdx.x;
        atomicAdd(&b.d_lens[(size_t)cam * 2 + (k - 21)], red[0][k] + red[1][k] + red[2][k] + red[3][k]);
    }
}

hipError_t mcn_launch_lens_ray_batch_bwd(const McnLensRayBatchBwdArgs& a, const McnSegTable& t, hipStream_t st) {
    int longest = 0;
    for (int k = 0; k < t.K; ++k) longest = max(longest, t.start[k + 1] - t.start[k]);
    if (longest <= 0) return hipSuccess;
    int gx = (longest + 255) / 256;
    if (gx > 512) gx = 512;
    hipLaunchKernelGGL(lens_ray_batch_bwd_kernel, dim3(gx, t.K), dim3(256), 0, st, a, t);
    return hipGetLastError();
}
