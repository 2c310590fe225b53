// The scene box fitted to the voxel sigma cache (`ray_bounds_fit = "voxel"`) for gfx950: the kernels of libmcnfit.so.
//
// "aabb" mode (ray_bounds.hip) samples every ray inside a box that somebody has to know; the sigma grid of "voxel" mode (voxel.hip)
// already says where the scene is.  This library draws the box from the grid on the device -- THE RULE is stated in
// include/mcnerf_fit.h -- and hands it to the ray-depth kernel as a device pointer: no value of it reaches the host.
//
// (1) voxel_box: three launches on the caller's stream.
//     fit_init_kernel    cells = (G, G, G, -1, -1, -1, 0, 0): the identities of the six minima / maxima.
//     fit_reduce_kernel  ONE pass over the grid, bandwidth-bound (226 MB at G = 384): 16-byte loads from the first 16-byte boundary on,
//                        at most 2048 workgroups and a grid-stride loop.  A thread keeps (ix, iy, iz) of its float4 and advances it by
//                        the stride's own (sx, sy, sz) with two carries, so the loop holds no division; four cells of one z-row (all but
//                        the float4s that straddle a row's end) cost four compares and six min / max.  The < 4 cells in front of the first
//                        boundary and the < 4 behind the last whole float4 go to the first threads of the grid.  Six integers per thread
//                        are reduced in the wave (ds_bpermute butterflies, once per kernel), across the four waves in LDS, and the
//                        workgroup issues at most six integer atomicMin / atomicMax on `cells` -- none when it saw no occupied cell, and
//                        none for a value that does not beat the one `cells` already holds (fit_peek).
//                        Integer min / max commute: two runs give the same bits.
//     fit_finish_kernel  steps (2) - (4) of the rule, one thread: status, and the six floats of `box` by ordinary stores.
// (2) ray_depths from a box on the device: ray_bounds.hip is compiled into this library as it stands (the library links none of another
//     library's objects), and fit_ray_depths_kernel is its per-ray device function behind six uniform loads -- nothing of the slab test or
//     of the rows is written here.
#include "mcnerf_scene_fit.h"
#include "ray_bounds.hip"

static constexpr int FIT_MAX_BLOCKS = 2048;      // 256 CUs x 8 workgroups: a memory-bound pass takes the rest by its grid-stride loop

struct FitRange { int lo[3], hi[3]; };

__device__ __forceinline__ void fit_take(FitRange& r, int ix, int iy, int iz) {
    r.lo[0] = min(r.lo[0], ix); r.hi[0] = max(r.hi[0], ix);
    r.lo[1] = min(r.lo[1], iy); r.hi[1] = max(r.hi[1], iy);
    r.lo[2] = min(r.lo[2], iz); r.hi[2] = max(r.hi[2], iz);
}
// one cell by its linear index (the ends of the grid only: this one divides)
__device__ __forceinline__ void fit_cell(FitRange& r, const McnVoxelBoxArgs& a, int i) {
    if (a.vox[i] > a.thresh) fit_take(r, i / (a.G * a.G), (i / a.G) % a.G, i % a.G);
}

// a value of `cells` as some earlier moment of this launch had it.  The minima only fall and the maxima only rise, so a workgroup whose
// value does not beat even that one has nothing to add and issues no atomic: 2048 workgroups' atomics on the same six words would
// otherwise queue up behind one another for longer than the pass over the grid takes
__device__ __forceinline__ int fit_peek(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(64) void fit_init_kernel(int* cells, int G) {
    if (threadIdx.x < 8) cells[threadIdx.x] = threadIdx.x < 3 ? G : threadIdx.x < 6 ? -1 : 0;
}

// head: cells in front of the first 16-byte boundary of vox (< 4); nvec: whole float4s from there on
__global__ __launch_bounds__(256) void fit_reduce_kernel(McnVoxelBoxArgs a, int head, int nvec) {
    __shared__ int part[4][6];
    const int G = a.G, total = G * G * G;
    const int T = gridDim.x * 256, t = blockIdx.x * 256 + threadIdx.x;
    const int tail = head + nvec * 4;
    FitRange r = {{G, G, G}, {-1, -1, -1}};
    if (t < head) fit_cell(r, a, t);
    if (t < total - tail) fit_cell(r, a, tail + t);
    const float4* v4 = reinterpret_cast<const float4*>(a.vox + head);
    const int i = head + 4 * t, s = 4 * T;                  // (i < 2^30 + 2^21: G <= 1024, at most 2048 workgroups)
    int ix = i / (G * G), iy = (i / G) % G, iz = i % G;
    const int sx = s / (G * G), sy = (s / G) % G, sz = s % G;
    for (int q = t; q < nvec; q += T) {
        const float4 v = v4[q];
        const bool o0 = v.x > a.thresh, o1 = v.y > a.thresh, o2 = v.z > a.thresh, o3 = v.w > a.thresh;
        if (o0 || o1 || o2 || o3) {
            if (iz + 3 < G) {                               // four cells of one z-row
                fit_take(r, ix, iy, iz + (o0 ? 0 : o1 ? 1 : o2 ? 2 : 3));
                r.hi[2] = max(r.hi[2], iz + (o3 ? 3 : o2 ? 2 : o1 ? 1 : 0));
            } else {                                        // the float4 straddles a row's end
                const bool o[4] = {o0, o1, o2, o3};
                int x = ix, y = iy, z = iz;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (o[e]) fit_take(r, x, y, z);
                    if (++z == G) { z = 0; if (++y == G) { y = 0; ++x; } }
                }
            }
        }
        iz += sz;
        int c = iz >= G ? 1 : 0;
        iz -= c ? G : 0;
        iy += sy + c;
        c = iy >= G ? 1 : 0;
        iy -= c ? G : 0;
        ix += sx + c;
    }
    // the wave's six values, then the workgroup's (every thread of the workgroup is here: nothing above returns)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            r.lo[k] = min(r.lo[k], __shfl_xor(r.lo[k], m, 64));
            r.hi[k] = max(r.hi[k], __shfl_xor(r.hi[k], m, 64));
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { part[wave][k] = r.lo[k]; part[wave][3 + k] = r.hi[k]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x, v = min(min(part[0][k], part[1][k]), min(part[2][k], part[3][k]));
        if (v < G && v < fit_peek(a.cells + k)) atomicMin(a.cells + k, v);
    } else if (threadIdx.x < 6) {
        const int k = threadIdx.x, v = max(max(part[0][k], part[1][k]), max(part[2][k], part[3][k]));
        if (v >= 0 && v > fit_peek(a.cells + k)) atomicMax(a.cells + k, v);
    }
}

__global__ __launch_bounds__(64) void fit_finish_kernel(McnVoxelBoxArgs a) {
    if (threadIdx.x != 0) return;
    const int m = min(a.margin, a.G);                       // (a margin of G or more pads to the whole grid; no i1 + margin overflows)
    int status = a.cells[3] >= 0 ? 1 : 0;
    float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3 && status != 0; ++k) {
        const int j0 = max(a.cells[k] - m, 0), j1 = min(a.cells[3 + k] + m, a.G - 1);
        v[k] = fmaxf(__fadd_rn(a.bmin, __fmul_rn((float)j0, a.h)), a.outer[k]);
        v[3 + k] = fminf(__fadd_rn(a.bmin, __fmul_rn((float)(j1 + 1), a.h)), a.outer[3 + k]);
        if (!(v[k] < v[3 + k])) status = 2;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) a.box[k] = status == 1 ? v[k] : a.outer[k];
    a.cells[6] = status;
    a.cells[7] = 0;
}

hipError_t mcn_launch_voxel_box(const McnVoxelBoxArgs& a, hipStream_t st) {
    const int total = a.G * a.G * a.G;
    const int lead = (int)(((16 - (reinterpret_cast<uintptr_t>(a.vox) & 15)) & 15) >> 2);
    const int head = lead < total ? lead : total, nvec = (total - head) / 4;
    const int want = (nvec + 255) / 256;
    const int blocks = want < 1 ? 1 : want > FIT_MAX_BLOCKS ? FIT_MAX_BLOCKS : want;
    hipLaunchKernelGGL(fit_init_kernel, dim3(1), dim3(64), 0, st, a.cells, a.G);
    hipLaunchKernelGGL(fit_reduce_kernel, dim3(blocks), dim3(256), 0, st, a, head, nvec);
    hipLaunchKernelGGL(fit_finish_kernel, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ the depths from a box on the device
__global__ __launch_bounds__(256) void fit_ray_depths_kernel(McnRayDepthsArgs a, const float* box) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { a.bmin[k] = box[k]; a.bmax[k] = box[3 + k]; }
    ray_depths_ray(a);
}
hipError_t mcn_launch_fit_ray_depths(const McnRayDepthsArgs& a, const float* box, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    hipLaunchKernelGGL(fit_ray_depths_kernel, dim3((a.N + 3) / 4), dim3(256), 0, st, a, box);
    return hipGetLastError();
}
