// Alpha-mask supervision of the FRONT weight for gfx950 (the extension library; include/mcnerf_ext.h):
//   fg[n] = sum_{j + 1 < S} w_j,  w_j the rgb composite's weights of composite.hip -- every weight but the far-plane sample's, whose
//   delta = 1e10 takes whatever transmittance is left (sum_j w_j is 1 on every ray);
// the composite backward that takes a gradient on fg beside the one on rgb; the gather of the drawn pixels' alpha; the MSE term.
//
// front_weight_kernel and composite_bwd_front_kernel follow composite_fwd_kernel / composite_bwd_kernel of composite.hip (a file this
// library does not touch): one wave per ray, grid-strided, the depths z = fl32(zrow[j] + jitter), a DPP inclusive product of u with a
// carry from chunk to chunk, the backward's two passes over LDS.  With d_fg null the backward IS that kernel's arithmetic and gives the
// bits of mcn_launch_composite_bwd, which tests/test_mask_ops_gpu.py asserts on every case: that is what keeps the two statements of
// the body together (defining it once: DESIGN.md 9).
//
// The mask path itself (front_weight, and the backward with d_fg) forms the per-sample quantities and the transmittance product in
// FP64 (mcn_sample64, wave_incl_prod_f64).  The fp32 form does not hold the feature's parity bar on semi-transparent rays of a
// thousand samples: u = 0.997 there, the device's expf near 1 is biased by -0.10 * 2^-24 (measured; the host's by +0.005), and the
// bias adds LINEARLY over the product -- 5e-6 in fg and 1e-5 in d_sig_rgb at S = 1024, five times the bar -- where rounding errors add
// as a random walk.  The weights are those of the colour composite to that difference (<= 6e-6 at S >= 1024, <= 6e-7 at S <= 128).
#include "mcnerf_mask.h"
#include "mcnerf_wave.h"

#define MCN_FRONT_BLOCKS 2048      // 4 waves each (as MCN_COMPOSITE_BLOCKS of composite.hip)

__device__ __forceinline__ float softplus_t(float x) {      // torch.nn.Softplus(beta=1, threshold=20)
    return x > 20.f ? x : log1pf(expf(x));
}
// (composite.hip: the running maximum of non-negative floats as bit patterns in one device word, the atomic skipped unless it raises it)
__device__ __forceinline__ void running_max_bits(unsigned* word, float v) {
    const unsigned mine = __float_as_uint(v);
    if (mine > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, mine);
}

// ---- the fp64 forms of the mask path
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

__global__ __launch_bounds__(256) void front_weight_kernel(McnFrontWeightArgs a) {
    const int lane = threadIdx.x & 63;
    const int S = a.S;
    for (int n = blockIdx.x * 4 + (threadIdx.x >> 6); n < a.N; n += gridDim.x * 4) {
    const float jit = a.jitter ? a.jitter[n] : 0.f;
    const float* zrow = a.zgrid + (size_t)n * a.z_stride;
    const float* sig = a.sig_rgb + (size_t)n * S * 4;      // component 0 of every sample: the colours are not read
    double carryT = 1.0, afg = 0.0;
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        const bool ok = j < S;
        McnSample64 s = {0.0, 1.0, 0.0};
        if (ok) s = mcn_sample64(sig[(size_t)j * 4], a.eps[(size_t)n * S + j], mcn_delta64(zrow, jit, j, S));
        const double inc = wave_incl_prod_f64(s.u);
        const double w = s.alpha * (carryT * wave_shr1_f64(inc, 1.0));
        carryT *= wave_last_f64(inc);
        if (j + 1 < S) afg += w;                            // every sample but the far-plane one
    }
    afg = wave_last_f64(wave_incl_sum_f64(afg));
    if (lane == 0) a.fg[n] = (float)afg;
    }
}

hipError_t mcn_launch_front_weight(const McnFrontWeightArgs& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    hipLaunchKernelGGL(front_weight_kernel, dim3(min((a.N + 3) / 4, MCN_FRONT_BLOCKS)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// composite_bwd_kernel (composite.hip): d alpha_j = dw_j T_j - (sum_{k>j} dw_k w_k) / u_j with dw_j = d_rgb . (c_j - wb), the per-ray
// intermediates staged in LDS (5 floats per sample per wave) between the prefix and the suffix pass -- word for word without d_fg.
// With d_fg the prefix pass forms T, u, e and w in fp64 (rounded once into the same LDS words; the suffix pass is the same) and
// d_fg[n] d fg / d alpha_j is added for j + 1 < S: what dw_j + d_fg would give, in a form that does not cancel (below).
__global__ __launch_bounds__(256) void composite_bwd_front_kernel(McnCompositeBwdFrontArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int S = a.S;
    float* sT = sm + (size_t)wv * 5 * S;
    float* sU = sT + S; float* sE = sU + S; float* sDW = sE + S; float* sDWW = sDW + S;
    float gmx = 0.f;
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
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        const bool ok = j < S;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (a.d_fg) {      // (a kernel argument: wave-uniform)  the mask path: the sample and the transmittance in fp64, see the top
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
    // the lanes (the DPP scans run one way)
    // The d_fg term is added to d alpha in closed form, last.  Put through dw it would be d_fg (T_j - sum_{j<k<S-1} w_k / u_j): where
    // the front is opaque the two are equal to a rounding and all that is left is their rounding noise (3e-8 absolute against a
    // gradient of 1e-4, measured).  But alpha_j T_j = T_j - T_{j+1} + 1e-10 T_j, so fg = 1 - T_{S-1} + 1e-10 sum_{j<S-1} T_j and
    //   d fg / d alpha_j = (T_{S-1} - 1e-10 sum_{j<k<S-1} T_k) / u_j   (j < S-1; 0 for the far sample),
    // which cancels nothing.  One more suffix scan, taken only with d_fg (a kernel argument: the branch is wave-uniform).
    const float Tfar = a.d_fg ? sT[S - 1] : 0.f;
    float carryR = 0.f, carryQ = 0.f;
    const int nch = (S + 63) / 64;
    for (int c = nch - 1; c >= 0; --c) {
        const int j = c * 64 + (63 - lane);
        const bool ok = j < S;
        const float inc = wave_incl_sum(ok ? sDWW[j] : 0.f);
        const float R = carryR + wave_shr1(inc, 0.f);
        carryR += wave_last(inc);
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

hipError_t mcn_launch_composite_bwd_front(const McnCompositeBwdFrontArgs& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    const size_t lds = (size_t)4 * 5 * a.S * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(composite_bwd_front_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(composite_bwd_front_kernel, dim3(min((a.N + 3) / 4, MCN_FRONT_BLOCKS)), dim3(256), lds, st, a);
    return hipGetLastError();
}

// alpha of the drawn pixels: one thread per ray, the camera from the by-value segment table
__global__ __launch_bounds__(256) void gather_alpha_kernel(McnGatherAlphaArgs a, McnSegTable tb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const long long pid = a.pix[i];
    float al = 1.f;
    if (pid < 0 || pid >= a.npix) {
        al = __uint_as_float(0x7fc00000u);                  // an id outside the image: nothing is read
    } else if (a.channels == 4) {
        const int cam = mcn_segment_of_ray(tb, i).cam;
        al = (float)a.images[((size_t)cam * (size_t)a.npix + (size_t)pid) * 4 + 3] / 255.0f;
    }
    a.alpha[i] = al;
}

hipError_t mcn_launch_gather_alpha(const McnGatherAlphaArgs& a, const McnSegTable& t, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_alpha_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a, t);
    return hipGetLastError();
}

// The mask term (train_loss_kernel's protocol, camera.hip): every block writes its slice of the gradients (they depend on no sum)
// and its partial of the squared error to out[4 + block]; the block that arrives last (counter in out[3], zero on entry, zero again
// on exit) adds the partials IN BLOCK ORDER and writes out[0..2].
__global__ __launch_bounds__(256) void mask_loss_kernel(const float* fg_c, const float* fg_f, const float* alpha, int n, float weight,
                                                       float* out, float* d_c, float* d_f) {
    __shared__ float red[256];
    __shared__ int last;
    const int t = threadIdx.x;
    const float gr = 2.f * weight / (float)n;
    float ar = 0.f;
    for (int i = blockIdx.x * 256 + t; i < n; i += gridDim.x * 256) {
        const float al = alpha[i], ec = fg_c[i] - al;
        ar += ec * ec;
        d_c[i] = gr * ec;
        if (fg_f) { const float ef = fg_f[i] - al; ar += ef * ef; d_f[i] = gr * ef; }
    }
    red[t] = ar;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) {
        out[4 + blockIdx.x] = red[0];
        __threadfence();
        last = atomicAdd(reinterpret_cast<unsigned*>(out + 3), 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last || t != 0) return;
    __threadfence();
    float sum = 0.f;
    for (int b = 0; b < (int)gridDim.x; ++b) sum += __builtin_nontemporal_load(out + 4 + b);       // (block order: deterministic)
    const float m = sum / (float)n;
    out[0] = weight * m; out[1] = m; out[2] = 0.f;
    *reinterpret_cast<unsigned*>(out + 3) = 0u;
}

hipError_t mcn_launch_mask_loss(const float* fg_c, const float* fg_f, const float* alpha, int n, float weight,
                                float* out, float* d_fg_c, float* d_fg_f, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    int blocks = (n + 1023) / 1024;
    if (blocks > MCN_MASK_LOSS_BLOCKS) blocks = MCN_MASK_LOSS_BLOCKS;
    hipLaunchKernelGGL(mask_loss_kernel, dim3(blocks), dim3(256), 0, st, fg_c, fg_f, alpha, n, weight, out, d_fg_c, d_fg_f);
    return hipGetLastError();
}
