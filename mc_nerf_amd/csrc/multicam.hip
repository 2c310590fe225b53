// The ray preamble of a MULTI-CAMERA train step (`cams_per_step` > 1, a sys_param key of this build): the batch is K
// segments of consecutive rays, segment k = n_k rays of camera cam_k.  One launch draws every segment's pixels, generates the rays
// from that camera's pose / inverse intrinsics and gathers the ground truth from that camera's resident uint8 image -- what
// sample_perm_kernel + raygen_fwd_kernel + gather_gt_kernel (select_raygen.hip) do for one camera in three launches, and with their
// bits.  Replaces MC_Model.get_rays + generate_rand_rays and the ground-truth gather (model/mc_nerf.py:124-145, 327-345, 379, 80)
// for a batch that spans cameras; the reference has no such step.
// The segment table travels by value in the kernel arguments (McnSegTable): no host-device copy, no host synchronisation.
//
// The per-ray device functions below RESTATE the arithmetic of the single-camera kernels, operation for operation.  They are not
// shared with select_raygen.hip: calling them from there re-ordered the operands of commutative instructions in sample_perm_kernel,
// raygen_fwd_kernel and raygen_bwd_kernel (scripts/device_code_diff.py: same results, other instruction streams), and those
// kernels' code objects stay as they are.  Every multiply / add that decides a bit is either an explicit __f*_rn or compiled with
// -ffp-contract=off, so equal text gives equal bits; tests/test_multicam_gpu.py holds the two files to torch.equal.
#include "mcnerf_multicam.h"

__device__ __forceinline__ unsigned mc_key(unsigned seed, unsigned i) {
    unsigned x = i * 0x9E3779B9u + seed;          // murmur3 finaliser: every output bit depends on every input bit
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

// P(i) of the keyed pseudo-random permutation P of [0, n): a 6-round balanced Feistel network on 2 * half bits (the smallest even
// width covering n) with the murmur finaliser as round function, cycle-walked back into [0, n).
// The key is the device word *seed plus `key_add` (mod 2^32; 0 for a single-camera draw).
__device__ __forceinline__ unsigned mcn_feistel_perm(unsigned i, unsigned n, const unsigned* seed, unsigned key_add) {
    int bits = 1;
    while (bits < 32 && (1ull << bits) < n) ++bits;
    const int half = (bits + 1) / 2;
    const unsigned mask = (1u << half) - 1u, sd = *seed + key_add;
    unsigned x = i;
    do {
        unsigned L = x >> half, R = x & mask;
#pragma unroll
        for (unsigned r = 0; r < 6; ++r) {
            const unsigned f = mc_key(sd + 0x632BE5ABu * (r + 1), R) & mask;
            const unsigned nl = R;
            R = L ^ f; L = nl;
        }
        x = (L << half) | R;
    } while (x >= n);
    return x;
}

// d = normalize(R^T K^-1 [u+.5, v+.5, 1]^T), o = -R^T t, following the reference's op order
// (pix @ K^-T, lift, @ pose_inv^T, minus origin, normalise) so results agree to ~1e-7.
// P [12] = world->cam [R|t] row-major, K [9] = inverse intrinsics; writes rays_d[i], rays_o[i] of the [n,3] outputs.
__device__ __forceinline__ void mcn_ray_of_pixel(const float* P, const float* K, long long pid, int W, float* rays_d, float* rays_o, int i) {
    const float u = (float)(pid % W) + 0.5f, v = (float)(pid / W) + 0.5f;
    float cam[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = __fadd_rn(__fadd_rn(__fmul_rn(u, K[r * 3]), __fmul_rn(v, K[r * 3 + 1])), K[r * 3 + 2]);
    float d[3], o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // pose_inv row c = [R[0][c], R[1][c], R[2][c], -(R^T t)[c]]
        const float ti = -(__fadd_rn(__fadd_rn(__fmul_rn(P[0 * 4 + c], P[3]), __fmul_rn(P[1 * 4 + c], P[7])), __fmul_rn(P[2 * 4 + c], P[11])));
        const float w = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(cam[0], P[0 * 4 + c]), __fmul_rn(cam[1], P[1 * 4 + c])), __fmul_rn(cam[2], P[2 * 4 + c])), ti);
        o[c] = ti;
        d[c] = __fsub_rn(w, ti);
    }
    const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) { rays_d[i * 3 + c] = d[c] / nrm; rays_o[i * 3 + c] = o[c]; }
}

// One ray's terms of the backward: acc[0..8] dR[j][c] from the direction, acc[9..17] dKinv[j][k], acc[18..20] the sum of the
// origin gradients (turned into pose terms once per block by mcn_raygen_bwd_flush).  Ray i of pix / d_rays_d / d_rays_o.
__device__ __forceinline__ void mcn_raygen_bwd_ray(const float* P, const float* K, const long long* pix, int W, const float* d_rays_d,
                                                   const float* d_rays_o, int i, float* acc) {
    const long long pid = pix[i];
    const float p[3] = {(float)(pid % W) + 0.5f, (float)(pid / W) + 0.5f, 1.f};
    float cam[3], q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = p[0] * K[r * 3] + p[1] * K[r * 3 + 1] + K[r * 3 + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = cam[0] * P[c] + cam[1] * P[4 + c] + cam[2] * P[8 + c];
    const float inv = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const float gd[3] = {d_rays_d[i * 3], d_rays_d[i * 3 + 1], d_rays_d[i * 3 + 2]};
    const float dn[3] = {q[0] * inv, q[1] * inv, q[2] * inv};
    const float dot = dn[0] * gd[0] + dn[1] * gd[1] + dn[2] * gd[2];
    float gq[3], gcam[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) gq[c] = (gd[c] - dn[c] * dot) * inv;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gcam[j] = P[j * 4] * gq[0] + P[j * 4 + 1] * gq[1] + P[j * 4 + 2] * gq[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[j * 3 + c] += cam[j] * gq[c];        // dR[j][c] from the direction
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[9 + j * 3 + k] += gcam[j] * p[k];     // dKinv[j][k]
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[18 + c] += d_rays_o[i * 3 + c];                        // sum of origin gradients
}

// Block reduction of the 21 accumulators of 256 threads (wave shuffle, then LDS) and one atomic per block and value into
// d_pose [12] / d_kinv [9] of the camera whose matrices are P (LDS).  red: __shared__ float [4][24].
__device__ __forceinline__ void mcn_raygen_bwd_flush(const float* acc, const float* P, float (*red)[24], float* d_pose, float* d_kinv) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 21; ++k) {
        float v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 21) {
        const int k = threadIdx.x;
        const float v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
        if (k < 9) atomicAdd(&d_pose[(k / 3) * 4 + (k % 3)], v);
        else if (k < 18) atomicAdd(&d_kinv[k - 9], v);
        else {
            // o_c = -sum_j R[j][c] t_j:  dR[j][c] += -t_j * Go_c ;  dt_j = -sum_c R[j][c] Go_c
            const int c = k - 18;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                atomicAdd(&d_pose[j * 4 + c], -P[j * 4 + 3] * v);
                atomicAdd(&d_pose[j * 4 + 3], -P[j * 4 + c] * v);
            }
        }
    }
}

// Ground-truth colour of one pixel of a uint8 image: rgb8/255 * a + (1 - a), a = alpha8/255 (RGBA composited on white,
// data/data_read.py:130-137; ToTensor's /255 first, then the blend in fp32, as the reference does), or rgb8/255 for 3 channels.
// Writes out[i] of the [n,3] output.
__device__ __forceinline__ void mcn_gt_of_pixel(const unsigned char* __restrict__ p, int channels, float* __restrict__ out, int i) {
    const float r = (float)p[0] / 255.0f, g = (float)p[1] / 255.0f, b = (float)p[2] / 255.0f;
    if (channels == 4) {
        const float a = (float)p[3] / 255.0f;
        out[i * 3 + 0] = r * a + (1.0f - a);
        out[i * 3 + 1] = g * a + (1.0f - a);
        out[i * 3 + 2] = b * a + (1.0f - a);
    } else {
        out[i * 3 + 0] = r; out[i * 3 + 1] = g; out[i * 3 + 2] = b;
    }
}

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
