// The distortion loss of mip-NeRF 360 on the rgb composite's weights for gfx950 (the regulariser library; include/mcnerf_reg.h,
// DESIGN.md 4i), per ray with S samples:
//   dist = sum_i sum_j w_i w_j |s_i - s_j|  +  (1/3) sum_{j < S-1} w_j^2 (s_{j+1} - s_j),   s_j = (z_j - z_near) z_scale,
// w_j the weights of composite.hip (same eps draw, same 1e-10, delta = 1e10 for the far sample, which takes part in the pair term at
// its depth and has NO interval term: its "interval" is the sentinel), and the composite backward that takes a gradient on dist
// beside the ones on rgb and on the front weight.
//
// The rows must be NON-DECREASING (the grid is, the pdf sampler's merged rows are): the kernels use the O(S) form.  With the
// exclusive prefix sums A_j = sum_{i<j} w_i, B_j = sum_{i<j} w_i s_i and the totals W = sum w, M = sum w s:
//   pair = 2 sum_j w_j (s_j A_j - B_j)
//   d dist / d w_j = 2 [ s_j (2 A_j + w_j - W) + M - 2 B_j - w_j s_j ]  +  (2/3) w_j (s_{j+1} - s_j) [j < S-1]
// Depths are constants of the backward: the gradient reaches sig_rgb through w only.
//
// distortion_fwd_kernel follows front_weight_kernel of mask.hip and composite_bwd_w_kernel RESTATES composite_bwd_front_kernel
// (files this library does not touch; defining the backward's body once for the three files: DESIGN.md 9): one wave per ray,
// grid-strided, z = fl32(zrow[j] + jitter), 64-sample chunks with carries, the backward's two passes over LDS.  Without d_dist the
// backward IS that kernel's arithmetic -- the bits of mcn_launch_composite_bwd_front, and without d_fg too those of
// mcn_launch_composite_bwd -- which tests/test_distortion_ops_gpu.py asserts on every case.
//
// The distortion path forms alpha, the transmittance product, w, s and both running sums in FP64 (the reason is mask.hip's: the
// device's fp32 expf near 1 is biased and the bias adds linearly over a thousand thin samples); s_j A_j - B_j is a difference of
// two O(1) sums that is O(delta) for neighbouring samples.  No atomics but the gmax word's: two runs give the same bits.
#include "mcnerf_distortion.h"
#include "mcnerf_wave.h"

#define MCN_DIST_BLOCKS 2048       // 4 waves each (as MCN_COMPOSITE_BLOCKS of composite.hip)

__device__ __forceinline__ float softplus_t(float x) {      // torch.nn.Softplus(beta=1, threshold=20)
    return x > 20.f ? x : log1pf(expf(x));
}
// (composite.hip: the running maximum of non-negative floats as bit patterns in one device word, the atomic skipped unless it raises it)
__device__ __forceinline__ void running_max_bits(unsigned* word, float v) {
    const unsigned mine = __float_as_uint(v);
    if (mine > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, mine);
}

// ---- the fp64 forms (mask.hip's, restated: that file belongs to another library)
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
// (mcnerf_wave.h's fp64 DPP move with an identity other than 0.0: out-of-range lanes keep `ident`)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_d_ident(double ident, double v) {
    const long long b = __double_as_longlong(v), o = __double_as_longlong(ident);
    const int lo = __builtin_amdgcn_update_dpp((int)o, (int)b, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double wave_incl_prod_f64(double v) {
    v *= dpp_d_ident<0x111, 0xf>(1.0, v); v *= dpp_d_ident<0x112, 0xf>(1.0, v); v *= dpp_d_ident<0x114, 0xf>(1.0, v);
    v *= dpp_d_ident<0x118, 0xf>(1.0, v); v *= dpp_d_ident<0x142, 0xa>(1.0, v); v *= dpp_d_ident<0x143, 0xc>(1.0, v);
    return v;
}
__device__ __forceinline__ double wave_shr1_f64(double v, double ident) { return dpp_d_ident<0x138, 0xf>(ident, v); }
// the exact fp64 difference of the two rounded fp32 depths of sample j, 1e10 for the far sample (j < S)
__device__ __forceinline__ double mcn_delta64(const float* zrow, float jit, int j, int S) {
    return (j + 1 < S) ? (double)__fadd_rn(zrow[j + 1], jit) - (double)__fadd_rn(zrow[j], jit) : 1e10;
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

__global__ __launch_bounds__(256) void distortion_fwd_kernel(McnDistortionFwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int S = a.S;
    const double zn = (double)a.z_near, zs = (double)a.z_scale;
    for (int n = blockIdx.x * 4 + (threadIdx.x >> 6); n < a.N; n += gridDim.x * 4) {
    const float jit = a.jitter ? a.jitter[n] : 0.f;
    const float* zrow = a.zgrid + (size_t)n * a.z_stride;
    const float* sig = a.sig_rgb + (size_t)n * S * 4;      // component 0 of every sample: the colours are not read
    double carryT = 1.0, carryA = 0.0, carryB = 0.0, acc = 0.0;
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        const bool ok = j < S;
        McnSample64 s = {0.0, 1.0, 0.0};
        double sj = 0.0, ds = 0.0;
        if (ok) {
            const double delta = mcn_delta64(zrow, jit, j, S);
            s = mcn_sample64(sig[(size_t)j * 4], a.eps[(size_t)n * S + j], delta);
            sj = ((double)__fadd_rn(zrow[j], jit) - zn) * zs;
            ds = (j + 1 < S) ? delta * zs : 0.0;             // the far sample has no interval term
        }
        const double inc = wave_incl_prod_f64(s.u);
        const double w = s.alpha * (carryT * wave_shr1_f64(inc, 1.0));
        carryT *= wave_last_f64(inc);
        const McnDistScan p = mcn_dist_scan(w, sj, carryA, carryB);
        acc += 2.0 * w * (sj * p.A - p.B) + (1.0 / 3.0) * (w * w) * ds;
    }
    acc = wave_last_f64(wave_incl_sum_f64(acc));
    if (lane == 0) {
        a.dist[n] = (float)acc;
        a.moments[(size_t)n * 2] = carryA;                  // W
        a.moments[(size_t)n * 2 + 1] = carryB;              // M
    }
    }
}

hipError_t mcn_launch_distortion_fwd(const McnDistortionFwdArgs& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    hipLaunchKernelGGL(distortion_fwd_kernel, dim3(min((a.N + 3) / 4, MCN_DIST_BLOCKS)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// composite_bwd_front_kernel (mask.hip), restated: d alpha_j = dw_j T_j - (sum_{k>j} dw_k w_k) / u_j with dw_j = d_rgb . (c_j - wb), the
// per-ray intermediates staged in LDS (5 floats per sample per wave) between the prefix and the suffix pass; with d_fg the prefix pass
// is fp64 and d_fg[n] d fg / d alpha_j is added in closed form -- word for word without d_dist.
// With d_dist the prefix pass is the fp64 one as well, forms A_j, B_j by fp64 scans (W, M from the forward's moments) and adds
// d_dist[n] d dist / d w_j to dw_j BEFORE sDW / sDWW are stored (dw and dw w are formed in fp64 and rounded once); the suffix sum of
// dw w then runs in fp64 over those words.  The d_fg term, when both are given, is the closed form unchanged.
__global__ __launch_bounds__(256) void composite_bwd_w_kernel(McnCompositeBwdWArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int S = a.S;
    float* sT = sm + (size_t)wv * 5 * S;
    float* sU = sT + S; float* sE = sU + S; float* sDW = sE + S; float* sDWW = sDW + S;
    float gmx = 0.f;
    const double zn = (double)a.z_near, zs = (double)a.z_scale;
    for (int n = blockIdx.x * 4 + wv; n < a.N; n += gridDim.x * 4) {
    const float jit = a.jitter ? a.jitter[n] : 0.f;
    const float* zrow = a.zgrid + (size_t)n * a.z_stride;
    const float g0 = a.d_rgb[n * 3], g1 = a.d_rgb[n * 3 + 1], g2 = a.d_rgb[n * 3 + 2];
    const float gf = a.d_fg ? a.d_fg[n] : 0.f;
    const float wb = a.white_back ? 1.f : 0.f;
    const f32x4* sr = reinterpret_cast<const f32x4*>(a.sig_rgb) + (size_t)n * S;
    f32x4* dst = reinterpret_cast<f32x4*>(a.d_sig_rgb) + (size_t)n * S;
    float carryT = 1.f;
    double carryT64 = 1.0;
    double gd = 0.0, Wt = 0.0, Mt = 0.0, carryA = 0.0, carryB = 0.0;
    if (a.d_dist) { gd = (double)a.d_dist[n]; Wt = a.moments[(size_t)n * 2]; Mt = a.moments[(size_t)n * 2 + 1]; }
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        const bool ok = j < S;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (a.d_dist) {    // (a kernel argument: wave-uniform)  the distortion path: mask.hip's fp64 prefix pass + the two sums
            McnSample64 s = {0.0, 1.0, 0.0};
            double sj = 0.0, ds = 0.0;
            if (ok) {
                v = sr[j];
                const double delta = mcn_delta64(zrow, jit, j, S);
                s = mcn_sample64(v[0], a.eps[(size_t)n * S + j], delta);
                sj = ((double)__fadd_rn(zrow[j], jit) - zn) * zs;
                ds = (j + 1 < S) ? delta * zs : 0.0;
            }
            const double inc = wave_incl_prod_f64(s.u);
            const double T = carryT64 * wave_shr1_f64(inc, 1.0);
            carryT64 *= wave_last_f64(inc);
            const double w64 = s.alpha * T;
            const McnDistScan p = mcn_dist_scan(w64, sj, carryA, carryB);
            if (ok) {
                const float w = (float)w64;
                const float dwc = g0 * (v[1] - wb) + g1 * (v[2] - wb) + g2 * (v[3] - wb);
                const double ddw = 2.0 * (sj * (2.0 * p.A + w64 - Wt) + Mt - 2.0 * p.B - w64 * sj) + (2.0 / 3.0) * w64 * ds;
                const double dw = (double)dwc + gd * ddw;
                sT[j] = (float)T; sU[j] = (float)s.u; sE[j] = (float)s.e; sDW[j] = (float)dw; sDWW[j] = (float)(dw * w64);
                float* o = reinterpret_cast<float*>(dst + j);
                const float o1 = w * g0, o2 = w * g1, o3 = w * g2;
                o[1] = o1;
                *reinterpret_cast<f32x2*>(o + 2) = (f32x2){o2, o3};
                gmx = fmaxf(gmx, fmaxf(fabsf(o1), fmaxf(fabsf(o2), fabsf(o3))));
            }
            continue;
        }
        if (a.d_fg) {      // (a kernel argument: wave-uniform)  the mask path: the sample and the transmittance in fp64
            McnSample64 s = {0.0, 1.0, 0.0};
            if (ok) {
                v = sr[j];
                s = mcn_sample64(v[0], a.eps[(size_t)n * S + j], mcn_delta64(zrow, jit, j, S));
            }
            const double inc = wave_incl_prod_f64(s.u);
            const double T = carryT64 * wave_shr1_f64(inc, 1.0);
            carryT64 *= wave_last_f64(inc);
            if (ok) {
                const float w = (float)(s.alpha * T);
                const float dw = g0 * (v[1] - wb) + g1 * (v[2] - wb) + g2 * (v[3] - wb);
                sT[j] = (float)T; sU[j] = (float)s.u; sE[j] = (float)s.e; sDW[j] = dw; sDWW[j] = dw * w;
                float* o = reinterpret_cast<float*>(dst + j);
                const float o1 = w * g0, o2 = w * g1, o3 = w * g2;
                o[1] = o1;
                *reinterpret_cast<f32x2*>(o + 2) = (f32x2){o2, o3};
                gmx = fmaxf(gmx, fmaxf(fabsf(o1), fmaxf(fabsf(o2), fabsf(o3))));
            }
            continue;
        }
        float delta = 0.f, e1 = 0.f;
        if (ok) {
            v = sr[j];
            const float z = __fadd_rn(zrow[j], jit);
            delta = (j + 1 < S) ? __fsub_rn(__fadd_rn(zrow[j + 1], jit), z) : 1e10f;
            e1 = a.eps[(size_t)n * S + j];
        }
        const float sx = v[0] + e1;
        const float sp = softplus_t(sx);
        const float ex = ok ? expf(-delta * sp) : 1.f;
        const float alpha = 1.f - ex;
        const float u = ok ? (1.f - alpha) + 1e-10f : 1.f;
        const float inc = wave_incl_prod(u);
        const float excl = wave_shr1(inc, 1.f);
        const float T = carryT * excl;
        carryT *= wave_last(inc);
        if (ok) {
            const float w = alpha * T;
            const float dw = g0 * (v[1] - wb) + g1 * (v[2] - wb) + g2 * (v[3] - wb);
            const float dsp = sx > 20.f ? 1.f : 1.f / (1.f + expf(-sx));      // d softplus
            sT[j] = T; sU[j] = u; sE[j] = ex * delta * dsp; sDW[j] = dw; sDWW[j] = dw * w;
            // components 1..3 only: component 0 (d sigma) belongs to the lane that takes sample j in the suffix pass
            float* o = reinterpret_cast<float*>(dst + j);
            const float o1 = w * g0, o2 = w * g1, o3 = w * g2;
            o[1] = o1;
            *reinterpret_cast<f32x2*>(o + 2) = (f32x2){o2, o3};
            gmx = fmaxf(gmx, fmaxf(fabsf(o1), fmaxf(fabsf(o2), fabsf(o3))));
        }
    }
    // pass 1's LDS writes are read below by OTHER lanes of this wave: the hardware executes one wave's LDS operations in issue
    // order, the fence + wave barrier keep the compiler from moving them across this line
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // suffix pass: lane l takes sample 63 - l of the chunk, so the sum of the samples AFTER a sample is an exclusive PREFIX scan over
    // the lanes (the DPP scans run one way).  The d_fg term is added to d alpha in closed form, last (mask.hip has the derivation):
    //   d fg / d alpha_j = (T_{S-1} - 1e-10 sum_{j<k<S-1} T_k) / u_j   (j < S-1; 0 for the far sample).
    const float Tfar = a.d_fg ? sT[S - 1] : 0.f;
    float carryR = 0.f, carryQ = 0.f;
    double carryR64 = 0.0;
    const int nch = (S + 63) / 64;
    for (int c = nch - 1; c >= 0; --c) {
        const int j = c * 64 + (63 - lane);
        const bool ok = j < S;
        float R;
        if (a.d_dist) {    // the distortion path: the suffix sum in fp64 (its terms change sign along the ray)
            const double inc = wave_incl_sum_f64(ok ? (double)sDWW[j] : 0.0);
            R = (float)(carryR64 + wave_shr1_f64(inc, 0.0));
            carryR64 += wave_last_f64(inc);
        } else {
            const float inc = wave_incl_sum(ok ? sDWW[j] : 0.f);
            R = carryR + wave_shr1(inc, 0.f);
            carryR += wave_last(inc);
        }
        float Q = 0.f;
        if (a.d_fg) {
            const float incq = wave_incl_sum(ok && j + 1 < S ? sT[j] : 0.f);
            Q = carryQ + wave_shr1(incq, 0.f);
            carryQ += wave_last(incq);
        }
        if (ok) {
            float dalpha = sDW[j] * sT[j] - R / sU[j];
            if (a.d_fg && j + 1 < S) dalpha += gf * ((Tfar - 1e-10f * Q) / sU[j]);      // (without d_fg nothing is added: not even a zero)
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

hipError_t mcn_launch_composite_bwd_w(const McnCompositeBwdWArgs& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    const size_t lds = (size_t)4 * 5 * a.S * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(composite_bwd_w_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(composite_bwd_w_kernel, dim3(min((a.N + 3) / 4, MCN_DIST_BLOCKS)), dim3(256), lds, st, a);
    return hipGetLastError();
}
