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
// distortion_fwd_kernel is the fp64 weight sweep of mcnerf_composite.h (front_weight_kernel's, mask.hip) with the two running sums,
// and composite_bwd_w_kernel the backward body defined there, which composite.hip and mask.hip compile too: one wave per ray,
// grid-strided, z = fl32(zrow[j] + jitter), 64-sample chunks with carries, the backward's two passes over LDS.  Without d_dist the
// backward is the instantiation of mask.hip -- the bits of mcn_launch_composite_bwd_front, and without d_fg too those of
// mcn_launch_composite_bwd -- which tests/test_distortion_ops_gpu.py asserts on every case.
//
// The distortion path forms alpha, the transmittance product, w, s and both running sums in FP64 (the reason is the sweep's: the
// device's fp32 expf near 1 is biased and the bias adds linearly over a thousand thin samples); s_j A_j - B_j is a difference of
// two O(1) sums that is O(delta) for neighbouring samples.  No atomics but the gmax word's: two runs give the same bits.
#include "mcnerf_distortion.h"
#include "mcnerf_composite.h"

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
        float sg = 0.f, e1 = 0.f;
        if (ok) { sg = sig[(size_t)j * 4]; e1 = a.eps[(size_t)n * S + j]; }
        const McnWeight64 q = mcn_weight_sweep64(sg, e1, zrow, jit, j, S, carryT);
        double sj = 0.0, ds = 0.0;
        if (ok) {
            sj = ((double)__fadd_rn(zrow[j], jit) - zn) * zs;
            ds = (j + 1 < S) ? q.delta * zs : 0.0;           // the far sample has no interval term
        }
        const double w = q.w;
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
    hipLaunchKernelGGL(distortion_fwd_kernel, dim3(min((a.N + 3) / 4, MCN_COMPOSITE_BLOCKS)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// The composite backward with gradients on the front weight and on dist beside the one on rgb (mcnerf_composite.h, which has the
// gradient formula at its place); FRONT: d_fg is given, DIST: d_dist is.
template <bool FRONT, bool DIST>
__global__ __launch_bounds__(256) void composite_bwd_w_kernel(McnCompositeBwdWArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    mcn_composite_bwd_rays<FRONT, DIST>({a.sig_rgb, a.zgrid, a.jitter, a.eps, a.d_rgb, a.d_fg, a.d_dist, a.moments, a.z_near, a.z_scale, a.N, a.S,
                                         a.white_back, a.d_sig_rgb, a.gmax_bits, a.z_stride}, sm);
}

hipError_t mcn_launch_composite_bwd_w(const McnCompositeBwdWArgs& a, hipStream_t st) {
    if (a.d_dist) return mcn_launch_composite_bwd_rays(a.d_fg ? composite_bwd_w_kernel<true, true> : composite_bwd_w_kernel<false, true>, a, st);
    return mcn_launch_composite_bwd_rays(a.d_fg ? composite_bwd_w_kernel<true, false> : composite_bwd_w_kernel<false, false>, a, st);
}
