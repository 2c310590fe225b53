// Per-ray sample bounds from an axis-aligned scene box (`ray_bounds = "aabb"`) for gfx950: the kernels of libmcnbox.so.
//
// The reference samples every ray on one global interval, linspace(near, far, S) (model/mc_nerf.py:598-611), and so did this build: a
// ray's samples beyond the scene box cost both MLPs and, in voxel mode, land in the border cells of the sigma grid (vox_axis clamps).
// Here every ray gets its own rows of depths: the model's grids mapped affinely onto [lo, hi], the part of [near, far] inside the box
// (slab test).  THE RULE is stated in include/mcnerf_box.h; every step is a separately rounded fp32 operation, so that a torch-CPU
// restatement gives the same bits, and a ray that the box does not clip gets a = 1, b = 0: fl(g[j] + jitter[n]), the bits the core
// kernels form from the shared grid.
//
// (1) ray_depths: one 64-lane wavefront per ray, four rays per workgroup of 256.  The ray's six floats are one broadcast read and its
//     (a, b) a few dozen instructions, formed by every lane of the wave alike; the wave then streams its rows out in 256-byte pieces
//     (768 B per ray at 64 + 128 depths, ~25 MB at 32768 rays: a write-bound streaming kernel).  No atomics, no LDS, no
//     data-dependent loop; every store is behind j < S of a ray behind n < N.
// (2) The inverse-CDF sampler and the voxel select / update reading their depths from rows [N,Sc], z_stride = Sc: the sampler's body
//     of mcnerf_sample_pdf.h under a kernel of this library's own, and the voxel kernels by compiling voxel.hip into this library as it
//     stands (the library links none of the core library's objects, voxel.o included).  The scan between a list's count and its write
//     comes the same way, with select.hip.
// The hit library (ray_skip.hip) compiles this file into itself in turn: box_ray_span returns the flag it forms, and ray_depths_kernel
// writes it where McnRayDepthsArgs::hit is given.  The fit library (scene_fit.hip) compiles it in as well, for ray_depths_ray.
#include "mcnerf_ray_bounds.h"
#include "mcnerf_sample_pdf.h"
#include "select.hip"
#include "voxel.hip"

__device__ __forceinline__ bool box_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// (lo, hi) of ray (o, d): the clipped interval, or (near, far); true iff the ray is CLIPPED
__device__ __forceinline__ bool box_ray_span(const McnRayDepthsArgs& a, const float* o, const float* d, float& lo, float& hi) {
    bool miss = false;
    float t_in = -INFINITY, t_out = INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float ok = o[k], dk = d[k];
        if (dk != 0.f) {                                     // (a NaN direction too: its t0, t1 are NaN)
            const float t0 = __fdiv_rn(__fsub_rn(a.bmin[k], ok), dk), t1 = __fdiv_rn(__fsub_rn(a.bmax[k], ok), dk);
            if (t0 != t0 || t1 != t1) miss = true;
            t_in = fmaxf(t_in, fminf(t0, t1));
            t_out = fminf(t_out, fmaxf(t0, t1));
        } else if (!(a.bmin[k] <= ok && ok <= a.bmax[k])) {
            miss = true;
        }
    }
    lo = fmaxf(a.z_near, t_in);
    hi = fminf(a.z_far, t_out);
    const bool clipped = !(miss || !box_finite(lo) || !box_finite(hi) || !(hi > lo));
    if (!clipped) { lo = a.z_near; hi = a.z_far; }
    return clipped;
}

// the wave's ray: its rows, span and flag.  The whole body of ray_depths_kernel, and of the fit library's kernel (scene_fit.hip), which
// first loads the box from the device into its copy of the arguments
__device__ __forceinline__ void ray_depths_ray(const McnRayDepthsArgs& a) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= a.N) return;
    float lo, hi;
    const bool clipped = box_ray_span(a, a.rays_o + (size_t)n * 3, a.rays_d + (size_t)n * 3, lo, hi);
    const float av = __fdiv_rn(__fsub_rn(hi, lo), __fsub_rn(a.z_far, a.z_near));
    const float bv = __fsub_rn(lo, __fmul_rn(av, a.z_near));
    const bool jit = a.jitter != nullptr;
    const float aj = jit ? __fmul_rn(av, a.jitter[n]) : 0.f;
    float* zc = a.z_c + (size_t)n * a.Sc;
    for (int j = lane; j < a.Sc; j += 64) {
        const float z = __fadd_rn(__fmul_rn(av, a.zgrid_c[j]), bv);
        zc[j] = jit ? __fadd_rn(z, aj) : z;
    }
    if (a.z_f) {
        float* zf = a.z_f + (size_t)n * a.Sf;
        for (int j = lane; j < a.Sf; j += 64) {
            const float z = __fadd_rn(__fmul_rn(av, a.zgrid_f[j]), bv);
            zf[j] = jit ? __fadd_rn(z, aj) : z;
        }
    }
    if (a.span && lane == 0) { a.span[(size_t)n * 2] = lo; a.span[(size_t)n * 2 + 1] = hi; }
    if (a.hit && lane == 0) a.hit[n] = clipped ? 1 : 0;
}
__global__ __launch_bounds__(256) void ray_depths_kernel(McnRayDepthsArgs a) { ray_depths_ray(a); }
hipError_t mcn_launch_ray_depths(const McnRayDepthsArgs& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    hipLaunchKernelGGL(ray_depths_kernel, dim3((a.N + 3) / 4), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ the sampler on rows
__global__ __launch_bounds__(256) void sample_pdf_rows_kernel(McnSamplePdfArgs a, int z_stride) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    mcn_sample_pdf_ray(a, z_stride, sm);
}
hipError_t mcn_launch_sample_pdf_rows(const McnSamplePdfArgs& a, hipStream_t st) {
    return mcn_launch_sample_pdf_kernel(sample_pdf_rows_kernel, a, st, a.Sc);
}

// ------------------------------------------------------------------ the voxel select / update on rows
// voxel.hip itself, compiled into this library (above): its kernels read z_stride from their arguments.  The scan between the count and
// the write is select.hip's, compiled into this library beside it (mcn_launch_select_scan on mcn_scan_counts, mcnerf_compact.h).
