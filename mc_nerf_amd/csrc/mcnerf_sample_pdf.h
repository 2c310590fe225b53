// The per-ray device code of the inverse-CDF sampler, defined once for the core library (sample_pdf.hip: depths from the shared grid) and
// the bounds library (ray_bounds.hip: one row of depths per ray).  The algorithm is stated in sample_pdf.hip.  The callers differ in
// z_stride alone: coarse depth j of ray n is zgrid[n * z_stride + j] + jitter[n] (z_stride 0: the shared grid; Sc: rows [N,Sc]), and
// z_stride is a parameter of the body, not a field of McnSamplePdfArgs: mcnerf_kernels.h is part of the source digest that ties the
// recorded MLP-kernel profiles to their sources and does not change with this.  (A header of its own, as mcnerf_voxel.h.)
#pragma once
#include "mcnerf_kernels.h"
#include "mcnerf_wave.h"

#define MCN_PDF_WAVES 4

// LDS of one wave, in floats: zc [Sc] | zs [I] | mid [Sc] | pdf [Sc] | cdf [Sc], each region rounded up to 4 floats.  The last
// three are dead once the samples are drawn and then hold the merge's Sc + 1 histogram counters.
static inline int pdf_r4(int x) { return (x + 3) & ~3; }
static inline size_t pdf_wave_floats(int Sc, int I) { return (size_t)4 * pdf_r4(Sc) + pdf_r4(I); }

// LDS written by some lanes of the wave and read by others: one wave's LDS operations execute in issue order, the fences + wave
// barrier keep the compiler from moving them across this point (composite.hip, backward)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// #{i < n : x[i] <= v} of a non-decreasing x (upper bound)
__device__ __forceinline__ int count_le(const float* x, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (x[m] <= v) lo = m + 1; else hi = m;
    }
    return lo;
}

// one 64-lane wavefront per ray, MCN_PDF_WAVES rays per workgroup; sm is the workgroup's dynamic LDS
__device__ __forceinline__ void mcn_sample_pdf_ray(const McnSamplePdfArgs& a, int z_stride, float* sm) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.x * MCN_PDF_WAVES + wv;
    if (n >= a.N) return;                                   // (the whole wave: nothing below synchronises the workgroup)
    const int Sc = a.Sc, I = a.I, T = Sc + I, nb = Sc - 2;
    const int Sc4 = (Sc + 3) & ~3;
    float* zc = sm + (size_t)wv * (4 * Sc4 + ((I + 3) & ~3));
    float* zs = zc + Sc4;
    float* mid = zs + ((I + 3) & ~3);
    float* pdf = mid + Sc4;
    float* cdf = pdf + Sc4;
    int* hist = reinterpret_cast<int*>(mid);
    const float jit = a.jitter ? a.jitter[n] : 0.f;
    const float* zrow = a.zgrid + (size_t)n * z_stride;
    const float* w = a.w + (size_t)n * Sc;

    // depths, edges and the floored weights (pdf[] holds wb until the total is known; each lane re-reads only its own entries)
    double tot = 0.0;
    for (int base = 0; base < Sc; base += 64) {
        const int j = base + lane;
        float wb = 0.f;
        if (j < Sc) {
            const float z = __fadd_rn(zrow[j], jit);
            zc[j] = z;
            if (j < Sc - 1) mid[j] = 0.5f * __fadd_rn(z, __fadd_rn(zrow[j + 1], jit));
            if (j < nb) { wb = __fadd_rn(w[j + 1], 1e-5f); pdf[j] = wb; }
        }
        tot += wave_last_f64(wave_incl_sum_f64((double)wb));
    }
    // pdf and its running sum
    const float totf = (float)tot;
    double carry = 0.0;
    if (lane == 0) cdf[0] = 0.f;
    for (int base = 0; base < nb; base += 64) {
        const int j = base + lane;
        float p = 0.f;
        if (j < nb) { p = pdf[j] / totf; pdf[j] = p; }
        const double inc = wave_incl_sum_f64((double)p);
        if (j < nb) cdf[j + 1] = (float)(carry + inc);
        carry += wave_last_f64(inc);
    }
    wave_lds_sync();

    // the importance samples
    const float* u = a.u + (size_t)n * I;
    for (int k = lane; k < I; k += 64) {
        const float uk = u[k];
        const int ind = count_le(cdf, Sc - 1, uk);
        const int below = ind - 1 > 0 ? ind - 1 : 0;
        const int above = ind < nb ? ind : nb;
        float denom = (ind >= 1 && ind <= nb) ? pdf[ind - 1] : 0.f;
        if (denom < 1e-5f) denom = 1.f;
        const float t = (uk - cdf[below]) / denom;
        zs[k] = mid[below] + t * (mid[above] - mid[below]);
    }
    wave_lds_sync();
    for (int c = lane; c <= Sc; c += 64) hist[c] = 0;
    wave_lds_sync();

    // merge by ranks: the samples ...
    float* out = a.z_all + (size_t)n * T;
    for (int k = lane; k < I; k += 64) {
        const float z = zs[k];
        const int c = count_le(zc, Sc, z);
        int r = 0;
        for (int q = 0; q < I; ++q) {
            const float v = zs[q];
            r += (v < z || (v == z && q < k)) ? 1 : 0;
        }
        out[c + r] = z;
        atomicAdd(&hist[c], 1);
    }
    wave_lds_sync();
    // ... and the coarse depths, each behind the samples that are smaller
    float below_n = 0.f;                                    // (counts <= 1024: exact in the float scan)
    for (int base = 0; base < Sc; base += 64) {
        const int j = base + lane;
        const float h = j < Sc ? (float)hist[j] : 0.f;
        const float inc = wave_incl_sum(h);
        if (j < Sc) out[j + (int)(below_n + inc)] = zc[j];
        below_n += wave_last(inc);
    }
}

// the launch of a kernel whose body is mcn_sample_pdf_ray: its LDS sizing and grid; `extra` follows the arguments
template <typename Kernel, typename... Extra>
hipError_t mcn_launch_sample_pdf_kernel(Kernel kernel, const McnSamplePdfArgs& a, hipStream_t st, Extra... extra) {
    if (a.N <= 0) return hipSuccess;
    const size_t lds = (size_t)MCN_PDF_WAVES * pdf_wave_floats(a.Sc, a.I) * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((a.N + MCN_PDF_WAVES - 1) / MCN_PDF_WAVES), dim3(64 * MCN_PDF_WAVES), lds, st, a, extra...);
    return hipGetLastError();
}
