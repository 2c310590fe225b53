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
//
// SELECT: count per ray -> exclusive scan (select_scan_kernel of select.hip) -> ordered write.  The list is in torch.nonzero
// (row-major) order and no atomic decides a position; the predicate is a gather vox[cell] > thresh (a NaN cell is empty).
//
// UPDATE, deterministic whatever the order of arrival: (1) every sample takes atomicMax of an order-preserving uint32 key of its
// sigma into a scratch grid (0 = none; every finite float's key is > 0; non-finite sigmas are skipped); (2) every sample atomicExch'es
// its cell's scratch word with 0 and the one thread that receives a non-zero key is the cell's single writer of
//   V <- (1 - beta) * V + beta * m      as  __fadd_rn(__fmul_rn(1 - beta, V), __fmul_rn(beta, m)),  1 - beta formed on the host.
// Untouched cells keep their bits, and the scratch grid is all zero again afterwards.
#include "mcnerf_voxel.h"
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
__device__ __forceinline__ size_t vox_sample_cell(const float* rays_o, const float* rays_d, const float* zgrid, const float* jitter,
                                                  int n, int j, float bmin, float s, int G) {
    const float z = jitter ? __fadd_rn(zgrid[j], jitter[n]) : zgrid[j];
    const float* o = rays_o + (size_t)n * 3;
    const float* d = rays_d + (size_t)n * 3;
    return vox_cell(__fadd_rn(o[0], __fmul_rn(d[0], z)), __fadd_rn(o[1], __fmul_rn(d[1], z)), __fadd_rn(o[2], __fmul_rn(d[2], z)), bmin, s, G);
}

// ------------------------------------------------------------------ select
// one wavefront per ray, four rays per workgroup (as select_count_kernel / select_write_kernel)
__global__ __launch_bounds__(256) void voxel_count_kernel(McnVoxelSelectArgs a) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= a.N) return;
    int cnt = 0;
    for (int base = 0; base < a.Sc; base += 64) {
        const int j = base + lane;
        const bool sel = j < a.Sc && a.vox[vox_sample_cell(a.rays_o, a.rays_d, a.zgrid, a.jitter, n, j, a.bmin, a.s, a.G)] > a.thresh;
        cnt += __popcll(__ballot(sel));
    }
    if (lane == 0) a.ray_counts[n] = cnt;
    if (a.out_c) {      // defaults for never-evaluated coarse samples (model/mc_nerf.py:689-694)
        f32x4 d; d[0] = a.sigma_default; d[1] = 1.f; d[2] = 1.f; d[3] = 1.f;
        f32x4* o = reinterpret_cast<f32x4*>(a.out_c) + (size_t)n * a.Sc;
        for (int j = lane; j < a.Sc; j += 64) o[j] = d;
    }
}
__global__ __launch_bounds__(256) void voxel_write_kernel(McnVoxelSelectArgs a) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= a.N) return;
    int pos = a.ray_offsets[n];
    for (int base = 0; base < a.Sc; base += 64) {
        const int j = base + lane;
        const bool sel = j < a.Sc && a.vox[vox_sample_cell(a.rays_o, a.rays_d, a.zgrid, a.jitter, n, j, a.bmin, a.s, a.G)] > a.thresh;
        const unsigned long long m = __ballot(sel);
        if (sel) a.idx[pos + __popcll(m & ((1ull << lane) - 1ull))] = make_int2(n, j);
        pos += __popcll(m);
    }
}
hipError_t mcn_launch_voxel_select(const McnVoxelSelectArgs& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    const dim3 g((a.N + 3) / 4), b(256);
    hipLaunchKernelGGL(voxel_count_kernel, g, b, 0, st, a);
    McnSelectArgs sc = {};
    sc.N = a.N; sc.ray_counts = a.ray_counts; sc.ray_offsets = a.ray_offsets; sc.count = a.count;
    hipError_t e = mcn_launch_select_scan(sc, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(voxel_write_kernel, g, b, 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ update (vox_key / vox_unkey: mcnerf_maxkey.h)
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
        cell = vox_sample_cell(a.rays_o, a.rays_d, a.zgrid, a.jitter, n, j, a.bmin, a.s, a.G);
        sig = a.sig_rgb[((size_t)n * a.Sc + j) * 4];
    }
    return (__float_as_uint(sig) & 0x7F800000u) != 0x7F800000u;
}
__global__ __launch_bounds__(256) void voxel_max_kernel(McnVoxelUpdateArgs a) {
    size_t cell; float sig;
    if (!vox_item(a, (long long)blockIdx.x * 256 + threadIdx.x, cell, sig)) return;
    atomicMax(&a.scratch[cell], vox_key(sig));
}
__global__ __launch_bounds__(256) void voxel_blend_kernel(McnVoxelUpdateArgs a) {
    size_t cell; float sig;
    if (!vox_item(a, (long long)blockIdx.x * 256 + threadIdx.x, cell, sig)) return;
    const unsigned k = atomicExch(&a.scratch[cell], 0u);
    if (k == 0u) return;                                    // another sample of this cell is its writer
    a.vox[cell] = __fadd_rn(__fmul_rn(a.one_minus_beta, a.vox[cell]), __fmul_rn(a.beta, vox_unkey(k)));
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
