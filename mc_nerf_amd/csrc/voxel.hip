// The voxel sigma cache of `coarse_sampler = "voxel"` for gfx950: a [G,G,G] fp32 grid of running raw (pre-softplus) coarse sigmas over
// the cube [bmin, bmax]^3 that prunes the coarse pass to the (ray, sample) pairs in occupied cells.
//
// The reference sketches the cache and never allocates it: NeRF_Model.query_sigma / update_sigma (model/mc_nerf.py:859-867) index a
// `sigma_voxels` tensor that does not exist, and inference(..., idx_render, coarse=True) (:682-704) already renders a coarse pass from
// a (ray, sample) list over a (sigma_default, 1, 1, 1) prefill (:689-694).  This file is the part that was missing.
//
// THE CELL OF A POINT p, per axis:  t = (p - bmin) * s,  s = float32(G) / float32(bmax - bmin) formed once on the host (no device
// division);  i = (int) min(max(t, 0), G - 1) -- fmaxf(NaN, 0) = 0, so a NaN lands in cell 0 and nothing indexes outside the grid;
// linear index (ix * G + iy) * G + iz in 64 bits.  Sample j of ray n sits at p = o + d * z, z = zgrid[j] + jitter[n], every step a
// separately rounded fp32 operation (as sample_pdf.hip forms its depths): the cell of a sample is a pure function of its inputs.
// With z_stride = Sc (McnVoxelSelectArgs / McnVoxelUpdateArgs) zgrid holds one row of depths per ray, z = zgrid[n * Sc + j] (+ jitter[n]):
// the bounds library (ray_bounds.hip) compiles this file into itself for its per-ray-rows entry points, so every kernel here exists once.
//
// SELECT: the ordered list compaction of mcnerf_compact.h with scale 1 under the predicate vox[cell] > thresh (a NaN cell is empty).
// UPDATE: the "max per cell, single writer" protocol of mcnerf_maxkey.h on the grid, an item being a sample and its raw sigma.
#include "mcnerf_voxel.h"
#include "mcnerf_compact.h"
#include "mcnerf_maxkey.h"

__device__ __forceinline__ int vox_axis(float p, float bmin, float s, int G) {
    const float t = __fmul_rn(__fsub_rn(p, bmin), s);
    return (int)fminf(fmaxf(t, 0.f), (float)(G - 1));
}
__device__ __forceinline__ size_t vox_cell(float x, float y, float z, float bmin, float s, int G) {
    const size_t ix = (size_t)vox_axis(x, bmin, s, G), iy = (size_t)vox_axis(y, bmin, s, G), iz = (size_t)vox_axis(z, bmin, s, G);
    return (ix * (size_t)G + iy) * (size_t)G + iz;
}
// the cell of sample j of ray n
__device__ __forceinline__ size_t vox_sample_cell(const float* rays_o, const float* rays_d, const float* zgrid, int z_stride, const float* jitter,
                                                  int n, int j, float bmin, float s, int G) {
    const float zr = zgrid[(size_t)n * z_stride + j];
    const float z = jitter ? __fadd_rn(zr, jitter[n]) : zr;
    const float* o = rays_o + (size_t)n * 3;
    const float* d = rays_d + (size_t)n * 3;
    return vox_cell(__fadd_rn(o[0], __fmul_rn(d[0], z)), __fadd_rn(o[1], __fmul_rn(d[1], z)), __fadd_rn(o[2], __fmul_rn(d[2], z)), bmin, s, G);
}

// ------------------------------------------------------------------ select
struct VoxelPred {
    const McnVoxelSelectArgs& a;
    __device__ __forceinline__ bool operator()(int n, int j) const {
        return a.vox[vox_sample_cell(a.rays_o, a.rays_d, a.zgrid, a.z_stride, a.jitter, n, j, a.bmin, a.s, a.G)] > a.thresh;
    }
};
// (templates, as select.hip's pair: the hit library runs them under VoxelPred behind a ray's hit flag, ray_skip.hip)
template <typename Pred, typename Args>
__global__ __launch_bounds__(256) void voxel_count_kernel(Args a) {
    mcn_compact_count<Pred>(a.N, a.Sc, 1, a.sigma_default, a.ray_counts, a.out_c, a);
}
template <typename Pred, typename Args>
__global__ __launch_bounds__(256) void voxel_write_kernel(Args a) {
    mcn_compact_write<Pred>(a.N, a.Sc, 1, a.ray_offsets, a.idx, a);
}
hipError_t mcn_launch_voxel_select(const McnVoxelSelectArgs& a, hipStream_t st) {
    return mcn_launch_compact<McnVoxelSelectArgs, voxel_count_kernel<VoxelPred, McnVoxelSelectArgs>, voxel_write_kernel<VoxelPred, McnVoxelSelectArgs>>(a, st);
}

// ------------------------------------------------------------------ update
// Item i of an update: its cell and its sigma.  false: nothing there (beyond the list, a pair outside [N) x [Sc), a non-finite sigma).
__device__ __forceinline__ bool vox_item(const McnVoxelUpdateArgs& a, long long i, size_t& cell, float& sig) {
    if (a.pts) {
        if (i >= a.M) return false;
        const float* p = a.pts + (size_t)i * 3;
        cell = vox_cell(p[0], p[1], p[2], a.bmin, a.s, a.G);
        sig = a.sigma[i];
    } else {
        int n, j;
        if (a.idx) {
            if (i >= min(*a.count, a.max_rows)) return false;
            const int2 e = a.idx[i];
            n = e.x; j = e.y;
            if ((unsigned)n >= (unsigned)a.N || (unsigned)j >= (unsigned)a.Sc) return false;
        } else {
            if (i >= (long long)a.N * a.Sc) return false;
            n = (int)(i / a.Sc); j = (int)(i - (long long)n * a.Sc);
        }
        cell = vox_sample_cell(a.rays_o, a.rays_d, a.zgrid, a.z_stride, a.jitter, n, j, a.bmin, a.s, a.G);
        sig = a.sig_rgb[((size_t)n * a.Sc + j) * 4];
    }
    return (__float_as_uint(sig) & 0x7F800000u) != 0x7F800000u;
}
__global__ __launch_bounds__(256) void voxel_max_kernel(McnVoxelUpdateArgs a) {
    mcn_cell_max(a.scratch, [&](long long i, size_t& cell, float& sig) { return vox_item(a, i, cell, sig); });
}
__global__ __launch_bounds__(256) void voxel_blend_kernel(McnVoxelUpdateArgs a) {
    mcn_cell_blend(a.vox, a.scratch, a.beta, a.one_minus_beta, [&](long long i, size_t& cell, float& sig) { return vox_item(a, i, cell, sig); });
}
hipError_t mcn_launch_voxel_update(const McnVoxelUpdateArgs& a, hipStream_t st) {
    const long long rows = a.pts ? a.M : (a.idx ? a.max_rows : (long long)a.N * a.Sc);
    if (rows <= 0) return hipSuccess;
    const dim3 g((unsigned)((rows + 255) / 256)), b(256);
    hipLaunchKernelGGL(voxel_max_kernel, g, b, 0, st, a);
    hipLaunchKernelGGL(voxel_blend_kernel, g, b, 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ query on explicit points
__global__ __launch_bounds__(256) void voxel_query_kernel(const float* vox, int G, float bmin, float s, const float* pts, int M, float* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float* p = pts + (size_t)i * 3;
    out[i] = vox[vox_cell(p[0], p[1], p[2], bmin, s, G)];
}
hipError_t mcn_launch_voxel_query(const float* vox, int G, float bmin, float s, const float* pts, int M, float* out, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(voxel_query_kernel, dim3((M + 255) / 256), dim3(256), 0, st, vox, G, bmin, s, pts, M, out);
    return hipGetLastError();
}
