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
// The per-ray body, its LDS layout and its launch are in mcnerf_sample_pdf.h (shared with the bounds library's per-ray-rows entry point).
#include "mcnerf_sample_pdf.h"

__global__ __launch_bounds__(256) void sample_pdf_kernel(McnSamplePdfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    mcn_sample_pdf_ray(a, 0, sm);
}

hipError_t mcn_launch_sample_pdf(const McnSamplePdfArgs& a, hipStream_t st) {
    return mcn_launch_sample_pdf_kernel(sample_pdf_kernel, a, st);
}
