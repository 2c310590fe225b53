// Ordered (ray, sample) list compaction, defined once for the fine-sample selection (select.hip) and the voxel-pruned coarse list
// (voxel.hip): count per ray -> exclusive scan (select_scan_kernel, select.hip) -> ordered write.  One wavefront per ray, four rays
// per workgroup of 256; a pass of the wave covers 64 samples, a ballot counts them and ranks the hits, and hit j of ray n goes behind
// ray_offsets[n] in sample order: the list is in torch.nonzero (row-major) order and no atomic decides a position.  The callers differ
// in the predicate Pred{a}(n, j) -> bool, built from the kernel's arguments behind the bounds check, and in `scale`: every hit is
// listed `scale` times, as (n, j * scale + r), r < scale (a literal 1 folds the loop away).  (A header of its own, as mcnerf_voxel.h.)
#pragma once
#include "mcnerf_kernels.h"

// ray_counts[n] = scale * hits of ray n; `out` (or null) is [N, S * scale] quads, prefilled here and nowhere else with the defaults of
// never-evaluated samples (sigma_default, 1, 1, 1) (model/mc_nerf.py:689-694)
template <typename Pred, typename Args>
__device__ __forceinline__ void mcn_compact_count(int N, int S, int scale, float sigma_default, int* ray_counts, float* out, const Args& a) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const Pred pred{a};
    int cnt = 0;
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        const bool sel = j < S && pred(n, j);
        cnt += __popcll(__ballot(sel));
    }
    if (lane == 0) ray_counts[n] = cnt * scale;
    if (out) {
        const int So = S * scale;
        f32x4 d; d[0] = sigma_default; d[1] = 1.f; d[2] = 1.f; d[3] = 1.f;
        f32x4* o = reinterpret_cast<f32x4*>(out) + (size_t)n * So;
        for (int j = lane; j < So; j += 64) o[j] = d;
    }
}
template <typename Pred, typename Args>
__device__ __forceinline__ void mcn_compact_write(int N, int S, int scale, const int* ray_offsets, int2* idx, const Args& a) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const Pred pred{a};
    int pos = ray_offsets[n];
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        const bool sel = j < S && pred(n, j);
        const unsigned long long m = __ballot(sel);
        if (sel) {
            int2* dst = idx + (pos + __popcll(m & ((1ull << lane) - 1ull)) * scale);
            for (int r = 0; r < scale; ++r) dst[r] = make_int2(n, j * scale + r);
        }
        pos += __popcll(m) * scale;
    }
}

// The body of the scan kernel (one workgroup of 1024; described at select_scan_kernel, select.hip): exclusive scan of ray_counts [N] ->
// ray_offsets [N], total -> *count.
__device__ __forceinline__ void mcn_scan_counts(int N, const int* ray_counts, int* ray_offsets, int* count) {
    __shared__ int wsum[16];
    constexpr int MAXQ = 16;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = (((N + 1023) / 1024) + 3) & ~3;
    const int lo = min(tid * per, N), hi = min(lo + per, N);
    const bool vec = per <= 4 * MAXQ && ((reinterpret_cast<size_t>(ray_counts) | reinterpret_cast<size_t>(ray_offsets)) & 15) == 0;
    int4 v[MAXQ];
    int s = 0;
    if (vec) {
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) {
            const int b = lo + 4 * q;
            int4 x = make_int4(0, 0, 0, 0);
            if (4 * q < per) {
                if (b + 3 < hi) x = *reinterpret_cast<const int4*>(ray_counts + b);
                else {
                    if (b < hi) x.x = ray_counts[b];
                    if (b + 1 < hi) x.y = ray_counts[b + 1];
                    if (b + 2 < hi) x.z = ray_counts[b + 2];
                }
            }
            v[q] = x;
        }
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) s += (v[q].x + v[q].y) + (v[q].z + v[q].w);
    } else {
        for (int i = lo; i < hi; ++i) s += ray_counts[i];
    }
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { const int t = wsum[w]; woff += w < wv ? t : 0; total += t; }
    int run = woff + inc - s;
    if (vec) {
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) {
            const int b = lo + 4 * q;
            if (4 * q < per && b < hi) {
                int4 o;
                o.x = run; run += v[q].x; o.y = run; run += v[q].y; o.z = run; run += v[q].z; o.w = run; run += v[q].w;
                if (b + 3 < hi) *reinterpret_cast<int4*>(ray_offsets + b) = o;
                else {
                    ray_offsets[b] = o.x;
                    if (b + 1 < hi) ray_offsets[b + 1] = o.y;
                    if (b + 2 < hi) ray_offsets[b + 2] = o.z;
                }
            }
        }
    } else {
        for (int i = lo; i < hi; ++i) { const int t = ray_counts[i]; ray_offsets[i] = run; run += t; }
    }
    if (tid == 0) *count = total;
}

// the scan alone (select.hip), N >= 1: ray_counts [N] -> exclusive ray_offsets [N], total -> *count
hipError_t mcn_launch_select_scan(int N, int* ray_counts, int* ray_offsets, int* count, hipStream_t st);

// count -> scan -> write on one stream; Args carries N, ray_counts, ray_offsets and count under these names
template <typename Args, void (*COUNT)(Args), void (*WRITE)(Args)>
hipError_t mcn_launch_compact(const Args& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    const dim3 g((a.N + 3) / 4), b(256);
    hipLaunchKernelGGL(COUNT, g, b, 0, st, a);
    const hipError_t e = mcn_launch_select_scan(a.N, a.ray_counts, a.ray_offsets, a.count, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(WRITE, g, b, 0, st, a);
    return hipGetLastError();
}
