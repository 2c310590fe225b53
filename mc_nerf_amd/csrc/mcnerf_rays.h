// The per-ray device arithmetic of the ray preamble, defined ONCE: the pixel permutation, the forward ray formula, the backward's
// per-ray terms and block flush, the ground-truth colour.  The single-camera kernels and the multi-camera ray-batch kernels (rays.hip)
// both call these functions, so they produce the same bits by construction.  Every multiply / add that decides a bit is either an
// explicit __f*_rn or compiled with -ffp-contract=off: do not re-associate an expression here.
// P [12] = one camera's world->cam [R|t] row-major and K [9] = its inverse intrinsics, in LDS or global memory.
#pragma once
#include "mcnerf_hash.h"

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

// mcn_ray_of_pixel in two halves, for a caller that changes `cam` between the lift and the rotation (the lens model of
// mcnerf_lens.h).  Each half repeats the expressions of mcn_ray_of_pixel above term for term: called back to back with `cam`
// unchanged they give its bits.
__device__ __forceinline__ void mcn_cam_of_pixel(const float* K, long long pid, int W, float* cam) {
    const float u = (float)(pid % W) + 0.5f, v = (float)(pid / W) + 0.5f;
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = __fadd_rn(__fadd_rn(__fmul_rn(u, K[r * 3]), __fmul_rn(v, K[r * 3 + 1])), K[r * 3 + 2]);
}
__device__ __forceinline__ void mcn_ray_of_cam(const float* P, const float* cam, float* rays_d, float* rays_o, int i) {
    float d[3], o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float ti = -(__fadd_rn(__fadd_rn(__fmul_rn(P[0 * 4 + c], P[3]), __fmul_rn(P[1 * 4 + c], P[7])), __fmul_rn(P[2 * 4 + c], P[11])));
        const float w = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(cam[0], P[0 * 4 + c]), __fmul_rn(cam[1], P[1 * 4 + c])), __fmul_rn(cam[2], P[2 * 4 + c])), ti);
        o[c] = ti;
        d[c] = __fsub_rn(w, ti);
    }
    const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) { rays_d[i * 3 + c] = d[c] / nrm; rays_o[i * 3 + c] = o[c]; }
}

// The part of mcn_raygen_bwd_ray below that depends on the lifted `cam` only, for the same caller: the direction's terms
// acc[0..8] dR[j][c] are accumulated and gcam [3], the gradient arriving at `cam`, is handed back (the caller turns it into the
// dKinv terms acc[9..17] and adds the origin gradients acc[18..20] itself).  The expressions are those of mcn_raygen_bwd_ray.
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
