// The device code of the ray preamble, defined ONCE: the pixel permutation, the forward ray formula, the backward's per-ray terms
// and block flush, the ground-truth colour, and the bodies of the ray-batch kernels.  The lens model is a compile-time option
// (template <bool LENS>; the undistortion itself is mcnerf_lens.h's): the single-camera kernels and the ray-batch kernels of rays.hip
// instantiate these functions without it, the kernels of lens.hip with it, so all produce the same bits by construction wherever the
// lens does not act.  Every multiply / add that decides a bit is either an explicit __f*_rn or compiled with -ffp-contract=off: do
// not re-associate an expression here.
// P [12] = one camera's world->cam [R|t] row-major, K [9] = its inverse intrinsics, L [2] = its lens coefficients (null without
// LENS), in LDS or global memory.
#pragma once
#include "mcnerf_hash.h"
#include "mcnerf_lens.h"

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
            const unsigned f = mcn_hash32(sd + 0x632BE5ABu * (r + 1), R) & mask;
            const unsigned nl = R;
            R = L ^ f; L = nl;
        }
        x = (L << half) | R;
    } while (x >= n);
    return x;
}

// The lift of a pixel through the inverse intrinsics: p = [u + 1/2, v + 1/2, 1]^T, cam = Kinv p, three rounded expressions.
__device__ __forceinline__ void mcn_cam_of_pixel(const float* K, long long pid, int W, float* p, float* cam) {
    const float u = (float)(pid % W) + 0.5f, v = (float)(pid / W) + 0.5f;
    p[0] = u; p[1] = v; p[2] = 1.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = __fadd_rn(__fadd_rn(__fmul_rn(u, K[r * 3]), __fmul_rn(v, K[r * 3 + 1])), K[r * 3 + 2]);
}
// d = normalize(R^T cam), o = -R^T t, following the reference's op order (lift, @ pose_inv^T, minus origin, normalise) so results
// agree to ~1e-7.  Writes rays_d[i], rays_o[i] of the [n,3] outputs.
__device__ __forceinline__ void mcn_ray_of_cam(const float* P, const float* cam, float* rays_d, float* rays_o, int i) {
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
// Ray i of pixel `pid`: the lift, with LENS the undistortion of mcnerf_lens.h by L [2] = (k1, k2), the rotation.
template <bool LENS>
__device__ __forceinline__ void mcn_ray_of_pixel(const float* P, const float* K, const float* L, long long pid, int W, float* rays_d, float* rays_o, int i) {
    float p[3], cam[3];
    mcn_cam_of_pixel(K, pid, W, p, cam);
    if constexpr (LENS) {
        float s, r;
        mcn_lens_undistort_cam(cam, L[0], L[1], &s, &r);
    }
    mcn_ray_of_cam(P, cam, rays_d, rays_o, i);
}

// The backward of mcn_ray_of_cam's direction: acc[0..8] += dR[j][c], and gcam [3] is the gradient arriving at `cam`.
__device__ __forceinline__ void mcn_raygen_bwd_cam(const float* P, const float* cam, const float* d_rays_d, int i, float* gcam, float* acc) {
    float q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = cam[0] * P[c] + cam[1] * P[4 + c] + cam[2] * P[8 + c];
    const float inv = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const float gd[3] = {d_rays_d[i * 3], d_rays_d[i * 3 + 1], d_rays_d[i * 3 + 2]};
    const float dn[3] = {q[0] * inv, q[1] * inv, q[2] * inv};
    const float dot = dn[0] * gd[0] + dn[1] * gd[1] + dn[2] * gd[2];
    float gq[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) gq[c] = (gd[c] - dn[c] * dot) * inv;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gcam[j] = P[j * 4] * gq[0] + P[j * 4 + 1] * gq[1] + P[j * 4 + 2] * gq[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[j * 3 + c] += cam[j] * gq[c];        // dR[j][c] from the direction
    }
}

// One ray's terms of the backward: acc[0..8] dR[j][c] from the direction (of the UNDISTORTED cam), acc[9..17] dKinv[j][k] (from the
// gradient at the lifted cam), acc[18..20] the sum of the origin gradients (turned into pose terms once per block by
// mcn_raygen_bwd_flush); with LENS also acc[21..22] d k1, d k2 of L [2].  Ray i of pix / d_rays_d / d_rays_o.
template <bool LENS>
__device__ __forceinline__ void mcn_raygen_bwd_ray(const float* P, const float* K, const float* L, const long long* pix, int W,
                                                   const float* d_rays_d, const float* d_rays_o, int i, float* acc) {
    float p[3], cam[3], gcam[3];
    mcn_cam_of_pixel(K, pix[i], W, p, cam);
    [[maybe_unused]] const float xd = cam[0], yd = cam[1];
    [[maybe_unused]] float s, r;
    if constexpr (LENS) mcn_lens_undistort_cam(cam, L[0], L[1], &s, &r);
    mcn_raygen_bwd_cam(P, cam, d_rays_d, i, gcam, acc);
    if constexpr (LENS) mcn_lens_undistort_bwd(xd, yd, s, r, L[0], L[1], gcam, acc + 21);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[9 + j * 3 + k] += gcam[j] * p[k];     // dKinv[j][k]
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[18 + c] += d_rays_o[i * 3 + c];            // sum of origin gradients
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

// ------------------------------------------------------------------ the bodies of the ray-batch kernels (rays.hip; lens.hip with LENS)
// Forward, one thread per ray i.  Its segment is found by mcn_segment_of_ray; the camera's 21 (+ 2) floats are read per ray through
// the cache: a block may straddle segments, so they cannot be staged once per block as raygen_fwd_kernel does.  The pixel is injected
// or drawn: segment k's own permutation of [0, H W), key *seed + k * 0x9E3779B9 (mod 2^32), so segment 0 draws what
// sample_perm_kernel draws.  lens [C,2] (null without LENS).
template <bool LENS>
__device__ __forceinline__ void mcn_ray_batch_fwd_body(const McnRayBatchArgs& a, const float* lens, const McnSegTable& t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const McnSegment g = mcn_segment_of_ray(t, i);
    const int k = g.k, cam = g.cam, lo = g.lo;
    const unsigned npix = (unsigned)a.H * (unsigned)a.W;
    const long long pid = a.pix_in ? a.pix_in[i] : (long long)mcn_feistel_perm((unsigned)(i - lo), npix, a.seed, (unsigned)k * 0x9E3779B9u);
    a.pix_out[i] = pid;
    mcn_ray_of_pixel<LENS>(a.pose + (size_t)cam * 12, a.kinv + (size_t)cam * 9, LENS ? lens + (size_t)cam * 2 : nullptr, pid, a.W, a.rays_d, a.rays_o, i);
    if (a.images) mcn_gt_of_pixel(a.images + ((size_t)cam * npix + (size_t)pid) * a.channels, a.channels, a.gt, i);
}

// Backward: blockIdx.y = segment.  A block grid-strides over its OWN segment only, so all its rays share one camera: the matrices
// (and coefficients) are staged in LDS and the 21 accumulators reduced as in raygen_bwd_kernel, then one atomic per block and value
// goes into that camera's rows of d_pose [C,3,4] / d_kinv [C,3,3] (a camera listed in two segments receives both; the caller zeroes
// the outputs).  With LENS the two lens sums ride in columns 21, 22 of `red`, which mcn_raygen_bwd_flush leaves alone (its barrier
// orders them too), into d_lens [C,2].  The block size is read with the builtin, not as blockDim.x: in a device function blockDim.x
// compiles to a choice between the size and the remainder of a partial last group, which only a __global__ function's body is
// relieved of (there the compiler knows the group size to be uniform); the launchers start full groups of 256.
template <bool LENS>
__device__ __forceinline__ void mcn_ray_batch_bwd_body(const McnRayBatchBwdArgs& a, const float* lens, float* d_lens, const McnSegTable& t) {
    constexpr int NACC = LENS ? 23 : 21;
    __shared__ float P[12], K[9], L[LENS ? 2 : 1];
    __shared__ float red[4][24];
    const int seg = blockIdx.y, cam = t.cam[seg], lo = t.start[seg], hi = t.start[seg + 1];
    const unsigned first = blockIdx.x * __builtin_amdgcn_workgroup_size_x();
    if (lo + (int)first >= hi) return;                               // (block-uniform: no ray of this segment for this block)
    if (threadIdx.x < 12) P[threadIdx.x] = a.pose[(size_t)cam * 12 + threadIdx.x];
    if (threadIdx.x < 9) K[threadIdx.x] = a.kinv[(size_t)cam * 9 + threadIdx.x];
    if constexpr (LENS) {
        if (threadIdx.x < 2) L[threadIdx.x] = lens[(size_t)cam * 2 + threadIdx.x];
    }
    __syncthreads();
    float acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
    for (int i = lo + first + threadIdx.x; i < hi; i += gridDim.x * __builtin_amdgcn_workgroup_size_x()) {
        mcn_raygen_bwd_ray<LENS>(P, K, L, a.pix, a.W, a.d_rays_d, a.d_rays_o, i, acc);
    }
    if constexpr (LENS) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
        for (int k = 21; k < 23; ++k) {
            float v = acc[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) red[wv][k] = v;
        }
    }
    mcn_raygen_bwd_flush(acc, P, red, a.d_pose + (size_t)cam * 12, a.d_kinv + (size_t)cam * 9);
    if constexpr (LENS) {
        if (threadIdx.x >= 21 && threadIdx.x < 23) {
            const int k = threadIdx.x;
            atomicAdd(&d_lens[(size_t)cam * 2 + (k - 21)], red[0][k] + red[1][k] + red[2][k] + red[3][k]);
        }
    }
}
