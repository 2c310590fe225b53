// Inverse-CDF hierarchical sampling for gfx950 (the fine sampler of `fine_sampler = "pdf"`): one 64-lane wavefront per ray,
// the ray's bins, CDF and samples in LDS, the CDF by wavefront prefix scans (mcnerf_wave.h).
//
// The reference has no such sampler (its fine pass is the weight-threshold refinement, model/mc_nerf.py:613-632); this is
// vanilla NeRF's sample_pdf in a deterministic form.  For ray n with Sc coarse samples and I = n_importance:
//   zc[j]  = zgrid[j] + jitter[n]                      (round to nearest: bit for bit the depths of the coarse pass)
//   mid[i] = 0.5 (zc[i] + zc[i+1]),  i < Sc-1          (bin edges)
//   wb[i]  = w[n, i+1] + 1e-5,        i < Sc-2          (interior weights, floored)
//   pdf    = wb / sum(wb),  cdf[0] = 0,  cdf[i+1] = cdf[i] + pdf[i]
//            (sum(wb) and every cdf entry are the correctly rounded sums: accumulated in fp64 by wavefront scans, rounded once to
//             fp32 -- up to the rare double rounding they do not depend on the order of the scan)
//   for each u = u[n, k]:  ind = #{i : cdf[i] <= u} (right-sided search),  below = max(ind-1, 0),  above = min(ind, Sc-2),
//                          denom = pdf[ind-1] when 1 <= ind <= Sc-2, else 0;  denom < 1e-5 -> 1,
//                          zs[k] = mid[below] + (u - cdf[below]) / denom * (mid[above] - mid[below])
//   z_all[n, :] = sort(zc ++ zs), ascending, Sc + I values (u may come in any order).
// THE denom RULE: denom is the bin's own pdf entry.  Vanilla NeRF takes it as cdf[above] - cdf[below]; near cdf = 0.5 that
// difference carries ~1 % error at 1e-5, so the `denom < 1e-5` branch would flip between two summation orders of the CDF.
// The pdf entry does not depend on the order, and the branch is decided by wb / sum(wb) alone.
//
// The sort is a merge by ranks: zc is sorted, so sample k lands at c_k + r_k, c_k = #{j : zc[j] <= zs[k]} (binary search),
// r_k = its rank among the zs (ties by index), and zc[j] at j + #{k : c_k <= j} (a histogram of the c_k, prefix-summed).
// Every position is < Sc + I whatever the inputs (NaN included), so a bad input garbles a row, never memory beyond it.
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

__global__ __launch_bounds__(256) void sample_pdf_kernel(McnSamplePdfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
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
    const float* w = a.w + (size_t)n * Sc;

    // depths, edges and the floored weights (pdf[] holds wb until the total is known; each lane re-reads only its own entries)
    double tot = 0.0;
    for (int base = 0; base < Sc; base += 64) {
        const int j = base + lane;
        float wb = 0.f;
        if (j < Sc) {
            const float z = __fadd_rn(a.zgrid[j], jit);
            zc[j] = z;
            if (j < Sc - 1) mid[j] = 0.5f * __fadd_rn(z, __fadd_rn(a.zgrid[j + 1], jit));
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

hipError_t mcn_launch_sample_pdf(const McnSamplePdfArgs& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    const size_t lds = (size_t)MCN_PDF_WAVES * pdf_wave_floats(a.Sc, a.I) * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_pdf_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(sample_pdf_kernel, dim3((a.N + MCN_PDF_WAVES - 1) / MCN_PDF_WAVES), dim3(64 * MCN_PDF_WAVES), lds, st, a);
    return hipGetLastError();
}
