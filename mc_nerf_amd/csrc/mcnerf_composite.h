// The alpha-compositing backward and the fp64 weight sweep of the one-wave-per-ray kernels, each defined once for the four
// libraries that run them: composite.hip (the core: fp32), mask.hip (the extension library: a gradient on the front weight),
// distortion.hip (the regulariser library: a gradient on the distortion loss) and depth.hip (the geometry library: a gradient on the
// expected depth).  Device code and the launch helper only; every library compiles its own instantiations.
//
// The mask, distortion and depth paths (mcn_weight_sweep64) and EVERY backward form the per-sample quantities and the
// transmittance product in FP64 (mcn_sample64, wave_incl_prod_f64).  The plain rgb backward had an fp32 prefix pass of its own: the
// sigma head's gradient, a sum over all samples that cancels 10- to 80-fold, came out 3e-4 of its value off an fp64 evaluation (at
// 8 and at 96 samples per ray alike; 1e-4 with this prefix pass, 4e-5 .. 9e-5 for torch's fp32 autograd on the same inputs).
// The fp32 form also does not hold the features' parity bar on
// semi-transparent rays of a thousand samples: u = 0.997 there, the device's expf near 1 is biased by -0.10 * 2^-24 (measured; the host's by +0.005), and the
// bias adds LINEARLY over the product -- 5e-6 in fg and 1e-5 in d_sig_rgb at S = 1024, five times the bar -- where rounding errors add
// as a random walk.  The weights are those of the colour composite to that difference (<= 6e-6 at S >= 1024, <= 6e-7 at S <= 128).
#pragma once
#include "mcnerf_wave.h"

#define MCN_COMPOSITE_BLOCKS 2048               // 4 waves each: 32 waves per CU, every ray-wave resident at once
#define MCN_COMPOSITE_BWD_MAX_SAMPLES 2048      // the backward's LDS: 4 waves x 5 floats per sample = 160 KiB at this S
static_assert((size_t)4 * 5 * MCN_COMPOSITE_BWD_MAX_SAMPLES * sizeof(float) <= 160 * 1024, "the backward's LDS at the bound");

__device__ __forceinline__ float softplus_t(float x) {      // torch.nn.Softplus(beta=1, threshold=20)
    return x > 20.f ? x : log1pf(expf(x));
}
// Running maximum of non-negative floats (as bit patterns) in ONE device word.  Every ray's wave contributes, and tens of
// thousands of same-address atomics serialise in the L2 (~150 us per launch at 32768 rays): read the word first with an
// L1-bypassing load and skip the atomic unless this wave would raise it -- after the first few waves almost none does.
// (A stale, lower value only costs a redundant atomic; the maximum never decreases.)
__device__ __forceinline__ void running_max_bits(unsigned* word, float v) {
    const unsigned mine = __float_as_uint(v);
    if (mine > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, mine);
}

// ---- the fp64 forms
// One sample in fp64 from its fp32 inputs: alpha = 1 - exp(-delta softplus(sigma + eps)) (as -expm1: no cancellation for a thin sample),
// u = 1 - alpha + 1e-10, and e = d alpha / d sigma_raw = exp(.) delta softplus'.  delta: the exact difference of the two fp32 depths.
struct McnSample64 { double alpha, u, e; };
__device__ __forceinline__ McnSample64 mcn_sample64(float sigma, float eps, double delta) {
    const double sx = (double)sigma + (double)eps;
    const double sp = sx > 20.0 ? sx : log1p(exp(sx));                          // torch.nn.Softplus(beta=1, threshold=20)
    const double alpha = -expm1(-delta * sp);
    const double ex = 1.0 - alpha;
    const double dsp = sx > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-sx));
    return {alpha, ex + 1e-10, ex * delta * dsp};
}
// the exact fp64 difference of the two rounded fp32 depths of sample j, 1e10 for the far sample (j < S)
__device__ __forceinline__ double mcn_delta64(const float* zrow, float jit, int j, int S) {
    return (j + 1 < S) ? (double)__fadd_rn(zrow[j + 1], jit) - (double)__fadd_rn(zrow[j], jit) : 1e10;
}

// One 64-sample chunk of the fp64 weight sweep, every lane of the wave active: sample j = base + lane of the row from its fp32
// inputs sigma, eps and the depth row (a lane past S reads no depth and carries alpha = 0, u = 1), the transmittance T by a DPP
// inclusive product of u with the carry from chunk to chunk, which then moves on by the chunk's product, and w = alpha T.
struct McnWeight64 { double T, w, u, e, delta; };
__device__ __forceinline__ McnWeight64 mcn_weight_sweep64(float sigma, float eps, const float* zrow, float jit, int j, int S, double& carryT) {
    McnSample64 s = {0.0, 1.0, 0.0};
    double delta = 0.0;
    if (j < S) {
        delta = mcn_delta64(zrow, jit, j, S);
        s = mcn_sample64(sigma, eps, delta);
    }
    const double inc = wave_incl_prod_f64(s.u);
    const double T = carryT * wave_shr1_f64(inc, 1.0);
    carryT *= wave_last_f64(inc);
    return {T, s.alpha * T, s.u, s.e, delta};
}

// One 64-sample chunk of the distortion sums, every lane of the wave active (a lane past S carries w = 0): the exclusive prefix sums
// A, B of this lane's sample from the chunk's inclusive fp64 scans and the carries, which then move on by the chunk's totals.
struct McnDistScan { double A, B; };
__device__ __forceinline__ McnDistScan mcn_dist_scan(double w, double s, double& carryA, double& carryB) {
    const double incA = wave_incl_sum_f64(w), incB = wave_incl_sum_f64(w * s);
    const McnDistScan r = {carryA + wave_shr1_f64(incA, 0.0), carryB + wave_shr1_f64(incB, 0.0)};
    carryA += wave_last_f64(incA);
    carryB += wave_last_f64(incB);
    return r;
}

// ---- the backward
struct McnCompositeBwdView {
    const float* sig_rgb;   // [N,S,4]
    const float* zgrid;     // [S] (z_stride 0) or [N,S] rows (z_stride S)
    const float* jitter;    // [N] or null
    const float* eps;       // [N,S]
    const float* d_rgb;     // [N,3]
    const float* d_fg;      // [N]; read with FRONT only
    const float* d_dist;    // [N]; read with DIST only, as moments, z_near and z_scale
    const double* moments;  // [N,2] = (W, M) of the distortion forward on the same inputs
    float z_near, z_scale;
    int N, S, white_back;
    float* d_sig_rgb;       // [N,S,4]
    unsigned* gmax_bits;    // or null
    int z_stride;
    const float* d_zexp;    // [N]; read with ZEXP only (the last member: a view built without it leaves it null)
};

// Backward of the rgb composite wrt (sigma_raw, rgb) of every sample:
//   rgb_out = sum_j w_j c_j (+ 1 - sum_j w_j),  w_j = alpha_j T_j,  T_j = prod_{k<j} u_k,  u = 1 - alpha + 1e-10
//   d alpha_j = dw_j T_j - (sum_{k>j} dw_k w_k) / u_j      (the cumprod gradient, division form)
// with dw_j = d_rgb . (c_j - wb).  Per-ray intermediates are staged in LDS (5 floats per sample per wave, `sm`) between the prefix
// and the suffix pass.  One wave per ray, grid-strided, in blocks of 4 waves.
// The prefix pass forms T, u, e and w in fp64 (rounded once into the LDS words; the suffix pass reads them as fp32).
// With FRONT d_fg[n] d fg / d alpha_j is added for j + 1 < S: what dw_j + d_fg would give, in a form that does not cancel (below).
// With DIST the prefix pass forms A_j, B_j by fp64 scans (W, M from the forward's moments) and adds
// d_dist[n] d dist / d w_j to dw_j BEFORE sDW / sDWW are stored (dw and dw w are formed in fp64 and rounded once); the suffix sum of
// dw w then runs in fp64 over those words.  The d_fg term, when both are given, is the closed form unchanged.
//   d dist / d w_j = 2 [ s_j (2 A_j + w_j - W) + M - 2 B_j - w_j s_j ]  +  (2/3) w_j (s_{j+1} - s_j) [j < S-1]      (distortion.hip)
// With ZEXP (the expected depth zexp = sum_j w_j z_j, depth.hip) the prefix pass is the fp64 one too and d_zexp[n] z_j is added to dw_j
// in fp64 before sDW / sDWW are stored; the suffix sum runs in fp64 as with DIST.
template <bool FRONT, bool DIST, bool ZEXP = false>
__device__ __forceinline__ void mcn_composite_bwd_rays(const McnCompositeBwdView& a, float* sm) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int S = a.S;
    float* sT = sm + (size_t)wv * 5 * S;
    float* sU = sT + S; float* sE = sU + S; float* sDW = sE + S; float* sDWW = sDW + S;
    float gmx = 0.f;                       // max |gradient| written by this lane (scale of the split-f16 backward)
    const double zn = (double)a.z_near, zs = (double)a.z_scale;
    for (int n = blockIdx.x * 4 + wv; n < a.N; n += gridDim.x * 4) {      // (several rays per wave: see the forward kernel)
    const float jit = a.jitter ? a.jitter[n] : 0.f;
    const float* zrow = a.zgrid + (size_t)n * a.z_stride;
    const float g0 = a.d_rgb[n * 3], g1 = a.d_rgb[n * 3 + 1], g2 = a.d_rgb[n * 3 + 2];
    const float gf = FRONT ? a.d_fg[n] : 0.f;
    const float wb = a.white_back ? 1.f : 0.f;
    const f32x4* sr = reinterpret_cast<const f32x4*>(a.sig_rgb) + (size_t)n * S;
    f32x4* dst = reinterpret_cast<f32x4*>(a.d_sig_rgb) + (size_t)n * S;
    double carryT64 = 1.0;
    double gd = 0.0, Wt = 0.0, Mt = 0.0, carryA = 0.0, carryB = 0.0;
    if constexpr (DIST) { gd = (double)a.d_dist[n]; Wt = a.moments[(size_t)n * 2]; Mt = a.moments[(size_t)n * 2 + 1]; }
    double gz = 0.0;
    if constexpr (ZEXP) gz = (double)a.d_zexp[n];
    // what sample j stages for the suffix pass, and its colour gradients
    auto stage = [&](int j, float T, float u, float e, float w, float dw, float dww) {
        sT[j] = T; sU[j] = u; sE[j] = e; sDW[j] = dw; sDWW[j] = dww;
        // components 1..3 only: component 0 (d sigma) belongs to the lane that takes sample j in the suffix pass
        float* o = reinterpret_cast<float*>(dst + j);
        const float o1 = w * g0, o2 = w * g1, o3 = w * g2;
        o[1] = o1;
        *reinterpret_cast<f32x2*>(o + 2) = (f32x2){o2, o3};
        gmx = fmaxf(gmx, fmaxf(fabsf(o1), fmaxf(fabsf(o2), fabsf(o3))));
    };
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        const bool ok = j < S;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        // the sample and the transmittance in fp64, see the top
        float e1 = 0.f;
        if (ok) { v = sr[j]; e1 = a.eps[(size_t)n * S + j]; }
        const McnWeight64 q = mcn_weight_sweep64(v[0], e1, zrow, jit, j, S, carryT64);
        double sj = 0.0, ds = 0.0;
        McnDistScan p = {0.0, 0.0};
        if constexpr (DIST) {          // + the two sums; the depths are constants of the backward
            if (ok) {
                sj = ((double)__fadd_rn(zrow[j], jit) - zn) * zs;
                ds = (j + 1 < S) ? q.delta * zs : 0.0;
            }
            p = mcn_dist_scan(q.w, sj, carryA, carryB);
        }
        if (ok) {
            const float w = (float)q.w;
            const float dwc = g0 * (v[1] - wb) + g1 * (v[2] - wb) + g2 * (v[3] - wb);
            if constexpr (DIST || ZEXP) {
                double dw = (double)dwc;
                if constexpr (DIST) {
                    const double ddw = 2.0 * (sj * (2.0 * p.A + q.w - Wt) + Mt - 2.0 * p.B - q.w * sj) + (2.0 / 3.0) * q.w * ds;
                    dw = (double)dwc + gd * ddw;
                }
                if constexpr (ZEXP) dw += gz * (double)__fadd_rn(zrow[j], jit);      // the depths are constants of the backward
                stage(j, (float)q.T, (float)q.u, (float)q.e, w, (float)dw, (float)(dw * q.w));
            } else {
                stage(j, (float)q.T, (float)q.u, (float)q.e, w, dwc, dwc * w);
            }
        }
    }
    // pass 1's LDS writes are read below by OTHER lanes of this wave: the hardware executes one wave's LDS operations in issue
    // order, the fence + wave barrier keep the compiler from moving them across this line
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // suffix pass: lane l takes sample 63 - l of the chunk, so the sum of the samples AFTER a sample is an exclusive PREFIX scan over
    // the lanes (the DPP scans run one way).
    // The d_fg term is added to d alpha in closed form, last.  Put through dw it would be d_fg (T_j - sum_{j<k<S-1} w_k / u_j): where
    // the front is opaque the two are equal to a rounding and all that is left is their rounding noise (3e-8 absolute against a
    // gradient of 1e-4, measured).  But alpha_j T_j = T_j - T_{j+1} + 1e-10 T_j, so fg = 1 - T_{S-1} + 1e-10 sum_{j<S-1} T_j and
    //   d fg / d alpha_j = (T_{S-1} - 1e-10 sum_{j<k<S-1} T_k) / u_j   (j < S-1; 0 for the far sample),
    // which cancels nothing.  One more suffix scan, taken only with FRONT.
    const float Tfar = FRONT ? sT[S - 1] : 0.f;
    float carryR = 0.f, carryQ = 0.f;
    double carryR64 = 0.0;
    const int nch = (S + 63) / 64;
    for (int c = nch - 1; c >= 0; --c) {
        const int j = c * 64 + (63 - lane);
        const bool ok = j < S;
        float R;                                                      // strictly later samples (of the chunk + of the chunks behind it)
        if constexpr (DIST || ZEXP) {      // the suffix sum in fp64 (with DIST its terms change sign along the ray)
            const double inc = wave_incl_sum_f64(ok ? (double)sDWW[j] : 0.0);
            R = (float)(carryR64 + wave_shr1_f64(inc, 0.0));
            carryR64 += wave_last_f64(inc);
        } else {
            const float inc = wave_incl_sum(ok ? sDWW[j] : 0.f);      // this sample and every later one of the chunk
            R = carryR + wave_shr1(inc, 0.f);
            carryR += wave_last(inc);
        }
        float Q = 0.f;
        if constexpr (FRONT) {
            const float incq = wave_incl_sum(ok && j + 1 < S ? sT[j] : 0.f);
            Q = carryQ + wave_shr1(incq, 0.f);
            carryQ += wave_last(incq);
        }
        if (ok) {
            float dalpha = sDW[j] * sT[j] - R / sU[j];
            if (FRONT && j + 1 < S) dalpha += gf * ((Tfar - 1e-10f * Q) / sU[j]);      // (without FRONT nothing is added: not even a zero)
            const float dsig = dalpha * sE[j];
            a.d_sig_rgb[((size_t)n * S + j) * 4] = dsig;
            gmx = fmaxf(gmx, fabsf(dsig));
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");         // the next ray's pass 1 rewrites the same LDS words
    __builtin_amdgcn_wave_barrier();
    }
    if (a.gmax_bits) {
        gmx = wave_max(gmx);
        if (lane == 0 && gmx < 3e38f) running_max_bits(a.gmax_bits, gmx);
    }
}

// The launch of a backward kernel (a __global__ wrapper of mcn_composite_bwd_rays) over N rays of S samples: the capped grid, the LDS
// of 4 waves x 5 floats per sample, opted in above 64 KiB.
template <typename Args>
hipError_t mcn_launch_composite_bwd_rays(void (*kernel)(Args), const Args& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    const size_t lds = (size_t)4 * 5 * a.S * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(min((a.N + 3) / 4, MCN_COMPOSITE_BLOCKS)), dim3(256), lds, st, a);
    return hipGetLastError();
}
