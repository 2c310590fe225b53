// Alpha compositing along rays for gfx950: one 64-lane wavefront per ray, samples strided over the
// lanes (coalesced float4 reads), transmittance by wavefront prefix scans (DPP), no LDS in
// the forward pass.  The backward's body is defined in mcnerf_composite.h, for this file and for the two feature libraries.
//
// Replaces the two composites of NeRF_Model.inference (model/mc_nerf.py:705-727) and
// NeRF_Model.sigma2weights (model/mc_nerf.py:729-736), plus the weights used for the fine-sample
// selection (model/mc_nerf.py:613-621).  The N(0,1) draws are inputs.
#include "mcnerf_kernels.h"
#include "mcnerf_composite.h"

__global__ __launch_bounds__(256) void composite_fwd_kernel(McnCompositeArgs a) {
    const int lane = threadIdx.x & 63;
    const int S = a.S;
    float wmx = 0.f;
    // a wave walks several rays (grid capped at MCN_COMPOSITE_BLOCKS): ONE running-maximum operation per wave, not per ray --
    // the waves' reads of that single device word serialise at its memory channel (32768 of them were most of the 45-65 us this
    // kernel took at 32768 rays)
    for (int n = blockIdx.x * 4 + (threadIdx.x >> 6); n < a.N; n += gridDim.x * 4) {
    const float jit = a.jitter ? a.jitter[n] : 0.f;
    const float* zrow = a.zgrid + (size_t)n * a.z_stride;
    const float dx = a.rays_d[n * 3], dy = a.rays_d[n * 3 + 1], dz = a.rays_d[n * 3 + 2];
    const float rlen = sqrtf(dx * dx + dy * dy + dz * dz);
    const f32x4* sr = reinterpret_cast<const f32x4*>(a.sig_rgb) + (size_t)n * S;
    float carryT = 1.f, carryTs = 1.f, carryCum = 0.f;
    float ar = 0.f, ag = 0.f, ab = 0.f, aw = 0.f, aop = 0.f, adep = 0.f;
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        const bool ok = j < S;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        float z = 0.f, delta = 0.f, e1 = 0.f, e2 = 0.f;
        if (ok) {
            v = sr[j];
            z = __fadd_rn(zrow[j], jit);
            delta = (j + 1 < S) ? __fsub_rn(__fadd_rn(zrow[j + 1], jit), z) : 1e10f;
            e1 = a.eps[(size_t)n * S + j];
            if (a.eps_sel) e2 = a.eps_sel[(size_t)n * S + j];
        }
        // rgb composite (sigma2weights)
        const float alpha = ok ? 1.f - expf(-delta * softplus_t(v[0] + e1)) : 0.f;
        const float u = ok ? (1.f - alpha) + 1e-10f : 1.f;
        const float inc = wave_incl_prod(u);
        const float excl = wave_shr1(inc, 1.f);
        const float w = alpha * (carryT * excl);
        carryT *= wave_last(inc);
        ar += w * v[1]; ag += w * v[2]; ab += w * v[3]; aw += w;
        // selection weights (independent noise draw)
        if (a.eps_sel) {
            const float al2 = ok ? 1.f - expf(-delta * softplus_t(v[0] + e2)) : 0.f;
            const float u2 = ok ? (1.f - al2) + 1e-10f : 1.f;
            const float inc2 = wave_incl_prod(u2);
            const float ex2 = wave_shr1(inc2, 1.f);
            const float w2 = al2 * (carryTs * ex2);
            carryTs *= wave_last(inc2);
            if (ok) { a.w_sel[(size_t)n * S + j] = w2; wmx = fmaxf(wmx, w2); }
        }
        // depth / opacity: noise-free, delta scaled by |d|, exp(-cumsum) transmittance
        if (a.depth) {
            const float sd = ok ? softplus_t(v[0]) * (delta * rlen) : 0.f;
            const float al3 = 1.f - expf(-sd);
            const float incs = wave_incl_sum(sd);
            const float exs = wave_shr1(incs, 0.f);   // exclusive sum by shift, never by subtraction: the last sample's sd (delta = 1e10) would cancel everything
            const float T = expf(-(carryCum + exs));
            carryCum += wave_last(incs);
            const float p = ok ? T * al3 : 0.f;
            aop += p; adep += z * p;
        }
    }
    ar = wave_sum(ar); ag = wave_sum(ag); ab = wave_sum(ab); aw = wave_sum(aw);
    if (a.depth) { aop = wave_sum(aop); adep = wave_sum(adep); }
    if (lane == 0) {
        if (a.white_back) { ar = (ar + 1.f) - aw; ag = (ag + 1.f) - aw; ab = (ab + 1.f) - aw; }
        a.rgb[n * 3] = ar; a.rgb[n * 3 + 1] = ag; a.rgb[n * 3 + 2] = ab;
        if (a.depth) { a.depth[n] = adep; a.opacity[n] = aop; }
    }
    }
    if (a.eps_sel && a.wmax_bits) {
        wmx = wave_max(wmx);
        if (lane == 0) running_max_bits(a.wmax_bits, wmx);
    }
}

hipError_t mcn_launch_composite_fwd(const McnCompositeArgs& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    hipLaunchKernelGGL(composite_fwd_kernel, dim3(min((a.N + 3) / 4, MCN_COMPOSITE_BLOCKS)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// The backward of the rgb composite wrt (sigma_raw, rgb) of every sample (mcnerf_composite.h: the fp32 form, no gradient on the
// front weight or on the distortion loss).
__global__ __launch_bounds__(256) void composite_bwd_kernel(McnCompositeBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    mcn_composite_bwd_rays<false, false>({a.sig_rgb, a.zgrid, a.jitter, a.eps, a.d_rgb, nullptr, nullptr, nullptr, 0.f, 0.f, a.N, a.S, a.white_back,
                                          a.d_sig_rgb, a.gmax_bits, a.z_stride}, sm);
}

hipError_t mcn_launch_composite_bwd(const McnCompositeBwdArgs& a, hipStream_t st) {
    return mcn_launch_composite_bwd_rays(composite_bwd_kernel, a, st);
}
