// The error-guided pixel sampler of `pixel_sampler = "error"` for gfx950: a [C, Th, Tw] fp32 map of running per-tile
// squared colour errors over the C training images (tiles of `tile` x `tile` pixels, edge tiles smaller) from which a train step
// draws its pixels in proportion to the error, and the map's update from the step's render.  The reference draws uniformly
// (model/mc_nerf.py:329); this is instant-ngp's error map on the segment table of the multi-camera step (mcnerf_multicam.h).
//
// TILE WEIGHTS are integers, so the CDF does not depend on the order of summation:
//   c_t = fminf(fmaxf(E_t, 0), 4)                          (NaN -> 0, +inf -> 4)
//   q_t = max(1, (uint64)(c_t * 2^24)) * area_t            (an exact power-of-two scaling, truncated; area_t = pixels of tile t)
// Pixel density is proportional to the clamped error, every tile keeps a non-zero weight (total > 0: no fallback branch), and
// total <= 4 * 2^24 * 2^26 = 2^52 is exact in a double.
//
// SAMPLE, two launches (the kernel boundary is the only ordering needed):
//   cdf    one block per segment k: inclusive uint64 prefix sums of q of camera cam[k] into cdf[k][0 .. T);
//   draw   one thread per ray; ray j of segment k (n_k rays) with uniforms (u0, u1), both clamped into [0, 1 - 2^-24] (NaN -> 0):
//          j < (int)((double)uniform_frac * n_k):  pix = min((int64)((double)u0 * (double)(H W)), H W - 1)      (uniform over the image)
//          otherwise: target = (uint64)((double)u0 * (double)total), tile = first t with cdf[k][t] > target, pixel
//          l = min((int)(u1 * (float)area_t), area_t - 1) of that tile in row-major order.  Draws are WITH replacement.
//
// UPDATE: the "max per cell, single writer" protocol of mcnerf_maxkey.h on the map, the cell of a ray being [cam, tile(pix)] and its
// value e = ((d0^2 + d1^2) + d2^2) * (1/3 in fp32), d = rgb - gt, every step a separately rounded fp32 operation.  Rays with a
// non-finite e or a pixel outside the image are skipped.
#include "mcnerf_errmap.h"
#include "mcnerf_maxkey.h"

#define ERR_CDF_ITEMS 8             // consecutive tiles a thread sums serially: one block scan covers 256 * 8 tiles

// rows and columns of tile (ty, tx): `tile`, or what is left of the image at its lower / right edge
__device__ __forceinline__ int err_tile_h(const McnErrGeom& g, int ty) { return min(g.tile, g.H - ty * g.tile); }
__device__ __forceinline__ int err_tile_w(const McnErrGeom& g, int tx) { return min(g.tile, g.W - tx * g.tile); }

__device__ __forceinline__ unsigned long long err_weight(const McnErrGeom& g, float E, int t) {
    const float c = fminf(fmaxf(E, 0.f), 4.f);
    unsigned long long q = (unsigned long long)__fmul_rn(c, 16777216.f);
    if (q < 1ull) q = 1ull;
    const int ty = t / g.Tw, tx = t - ty * g.Tw;
    return q * (unsigned long long)(err_tile_h(g, ty) * err_tile_w(g, tx));
}

// ------------------------------------------------------------------ sample
__global__ __launch_bounds__(256) void errmap_cdf_kernel(McnErrSampleArgs a, McnSegTable t) {
    __shared__ unsigned long long sh[2][256];
    const int tid = threadIdx.x, k = blockIdx.x, T = a.g.T;
    const float* E = a.err + (size_t)t.cam[k] * T;
    unsigned long long* out = a.cdf + (size_t)k * T;
    unsigned long long carry = 0;
    for (int base = 0; base < T; base += 256 * ERR_CDF_ITEMS) {
        const int lo = base + tid * ERR_CDF_ITEMS;
        unsigned long long q[ERR_CDF_ITEMS], s = 0;
#pragma unroll
        for (int i = 0; i < ERR_CDF_ITEMS; ++i) {
            q[i] = lo + i < T ? err_weight(a.g, E[lo + i], lo + i) : 0ull;
            s += q[i];
        }
        int cur = 0;                                        // inclusive scan of the 256 chunk sums through LDS
        sh[0][tid] = s;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            unsigned long long v = sh[cur][tid];
            if (tid >= off) v += sh[cur][tid - off];
            sh[cur ^ 1][tid] = v;
            cur ^= 1;
            __syncthreads();
        }
        unsigned long long run = carry + sh[cur][tid] - s;
        carry += sh[cur][255];
#pragma unroll
        for (int i = 0; i < ERR_CDF_ITEMS; ++i)
            if (lo + i < T) { run += q[i]; out[lo + i] = run; }
        __syncthreads();                                    // (the next chunk writes sh[0] again)
    }
}
__device__ __forceinline__ float err_unit(float u) { return fminf(fmaxf(u, 0.f), 0.99999994f); }     // [0, 1 - 2^-24]; NaN -> 0
__global__ __launch_bounds__(256) void errmap_draw_kernel(McnErrSampleArgs a, McnSegTable t) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const McnErrGeom& g = a.g;
    const int k = mcn_segment_of_ray(t, i).k;              // (this kernel takes the number only and indexes the table with it, as it always did)
    const int j = i - t.start[k], nk = t.start[k + 1] - t.start[k];
    const int n_u = (int)((double)a.uniform_frac * (double)nk);
    const float u0 = err_unit(a.u[(size_t)i * 2]), u1 = err_unit(a.u[(size_t)i * 2 + 1]);
    const long long npix = (long long)g.H * g.W;
    long long pix;
    if (j < n_u) {
        pix = min((long long)((double)u0 * (double)npix), npix - 1);
    } else {
        const unsigned long long* cdf = a.cdf + (size_t)k * g.T;
        const unsigned long long target = (unsigned long long)((double)u0 * (double)cdf[g.T - 1]);
        int lo = 0, hi = g.T - 1;                           // first tile with cdf > target, clamped to T - 1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] > target) hi = mid; else lo = mid + 1;
        }
        const int ty = lo / g.Tw, tx = lo - ty * g.Tw;
        const int tw = err_tile_w(g, tx), area = err_tile_h(g, ty) * tw;
        const int l = min((int)__fmul_rn(u1, (float)area), area - 1);
        const int r = l / tw;
        pix = (long long)(ty * g.tile + r) * g.W + tx * g.tile + (l - r * tw);
    }
    a.pix[i] = pix;
}
hipError_t mcn_launch_errmap_sample(const McnErrSampleArgs& a, const McnSegTable& t, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(errmap_cdf_kernel, dim3(t.K), dim3(256), 0, st, a, t);
    hipLaunchKernelGGL(errmap_draw_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a, t);
    return hipGetLastError();
}

// ------------------------------------------------------------------ update
// Ray i of an update: its map cell and its error.  false: nothing there (beyond the batch, a pixel outside the image, a non-finite e).
__device__ __forceinline__ bool err_item(const McnErrUpdateArgs& a, const McnSegTable& t, int i, size_t& cell, float& e) {
    if (i >= a.n) return false;
    const McnErrGeom& g = a.g;
    const long long p = a.pix[i];
    if (p < 0 || p >= (long long)g.H * g.W) return false;
    const float* c = a.rgb + (size_t)i * 3;
    const float* w = a.gt + (size_t)i * 3;
    const float d0 = __fsub_rn(c[0], w[0]), d1 = __fsub_rn(c[1], w[1]), d2 = __fsub_rn(c[2], w[2]);
    e = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)), 0.333333343f);
    const int y = (int)(p / g.W), x = (int)(p - (long long)y * g.W);
    cell = (size_t)t.cam[mcn_segment_of_ray(t, i).k] * g.T + (size_t)(y / g.tile) * g.Tw + (size_t)(x / g.tile);
    return (__float_as_uint(e) & 0x7F800000u) != 0x7F800000u;
}
__global__ __launch_bounds__(256) void errmap_max_kernel(McnErrUpdateArgs a, McnSegTable t) {
    mcn_cell_max(a.scratch, [&](int i, size_t& cell, float& e) { return err_item(a, t, i, cell, e); });
}
__global__ __launch_bounds__(256) void errmap_blend_kernel(McnErrUpdateArgs a, McnSegTable t) {
    mcn_cell_blend(a.err, a.scratch, a.beta, a.one_minus_beta, [&](int i, size_t& cell, float& e) { return err_item(a, t, i, cell, e); });
}
hipError_t mcn_launch_errmap_update(const McnErrUpdateArgs& a, const McnSegTable& t, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    const dim3 g((a.n + 255) / 256), b(256);
    hipLaunchKernelGGL(errmap_max_kernel, g, b, 0, st, a, t);
    hipLaunchKernelGGL(errmap_blend_kernel, g, b, 0, st, a, t);
    return hipGetLastError();
}
