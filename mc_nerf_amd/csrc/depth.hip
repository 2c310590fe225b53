// Depth supervision of the training render for gfx950 (the geometry library; include/mcnerf_geo.h), per ray with S samples:
//   zexp[n] = sum_{j=0}^{S-1} w_j z_j,   z_j = fl32(zrow[j] + jitter[n]),
// w_j the rgb composite's weights of composite.hip (same eps draw, same 1e-10, delta not scaled by |d|, 1e10 for the far sample, which
// takes part at its depth z_{S-1}: it holds the transmittance that is left); the composite backward that takes a gradient on zexp
// beside the ones on rgb, on the front weight and on the distortion term; the gather of the drawn pixels' depth targets; the MSE term
// over the rays that have a measurement.  Depths are constants of the backward: the gradient reaches sig_rgb through w only.
//
// depth_fwd_kernel is the fp64 weight sweep of mcnerf_composite.h (front_weight_kernel's, mask.hip) with sum w z accumulated in fp64 and
// rounded once, and composite_bwd_z_kernel the backward body defined there, which composite.hip, mask.hip and distortion.hip compile
// too: one wave per ray, grid-strided, 64-sample chunks with carries, the backward's two passes over LDS.  Without d_zexp the backward
// is the instantiation of distortion.hip -- the bits of mcn_launch_composite_bwd_w -- which tests/test_depth_ops_gpu.py asserts on every
// case.  The reason for the sweep's fp64 is told in mcnerf_composite.h.  No atomics but the gmax word's and the loss's integer arrival
// counter: two runs give the same bits.
#include "mcnerf_depth.h"
#include "mcnerf_composite.h"

__global__ __launch_bounds__(256) void depth_fwd_kernel(McnDepthFwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int S = a.S;
    for (int n = blockIdx.x * 4 + (threadIdx.x >> 6); n < a.N; n += gridDim.x * 4) {
    const float jit = a.jitter ? a.jitter[n] : 0.f;
    const float* zrow = a.zgrid + (size_t)n * a.z_stride;
    const float* sig = a.sig_rgb + (size_t)n * S * 4;      // component 0 of every sample: the colours are not read
    double carryT = 1.0, acc = 0.0;
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        float sg = 0.f, e1 = 0.f;
        if (j < S) { sg = sig[(size_t)j * 4]; e1 = a.eps[(size_t)n * S + j]; }
        const McnWeight64 q = mcn_weight_sweep64(sg, e1, zrow, jit, j, S, carryT);
        if (j < S) acc += q.w * (double)__fadd_rn(zrow[j], jit);      // the far-plane sample included, at its depth
    }
    acc = wave_last_f64(wave_incl_sum_f64(acc));
    if (lane == 0) a.zexp[n] = (float)acc;
    }
}

hipError_t mcn_launch_depth_fwd(const McnDepthFwdArgs& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    hipLaunchKernelGGL(depth_fwd_kernel, dim3(min((a.N + 3) / 4, MCN_COMPOSITE_BLOCKS)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// The composite backward with gradients on the front weight, on dist and on zexp beside the one on rgb (mcnerf_composite.h, which has
// the gradient formulas at their place); FRONT: d_fg is given, DIST: d_dist is, ZEXP: d_zexp is.
template <bool FRONT, bool DIST, bool ZEXP>
__global__ __launch_bounds__(256) void composite_bwd_z_kernel(McnCompositeBwdZArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    mcn_composite_bwd_rays<FRONT, DIST, ZEXP>({a.sig_rgb, a.zgrid, a.jitter, a.eps, a.d_rgb, a.d_fg, a.d_dist, a.moments, a.z_near, a.z_scale, a.N, a.S,
                                               a.white_back, a.d_sig_rgb, a.gmax_bits, a.z_stride, a.d_zexp}, sm);
}

template <bool ZEXP>
static hipError_t launch_bwd_z(const McnCompositeBwdZArgs& a, hipStream_t st) {
    if (a.d_dist) return mcn_launch_composite_bwd_rays(a.d_fg ? composite_bwd_z_kernel<true, true, ZEXP> : composite_bwd_z_kernel<false, true, ZEXP>, a, st);
    return mcn_launch_composite_bwd_rays(a.d_fg ? composite_bwd_z_kernel<true, false, ZEXP> : composite_bwd_z_kernel<false, false, ZEXP>, a, st);
}

hipError_t mcn_launch_composite_bwd_z(const McnCompositeBwdZArgs& a, hipStream_t st) {
    return a.d_zexp ? launch_bwd_z<true>(a, st) : launch_bwd_z<false>(a, st);
}

// a depth target is a measurement iff it is finite and > 0
__device__ __forceinline__ bool depth_valid(float d) { return d > 0.f && d <= 3.4028234664e38f; }

// the targets of the drawn pixels: one thread per ray, the camera from the by-value segment table; no measurement -> 0
__global__ __launch_bounds__(256) void gather_depth_kernel(McnGatherDepthArgs a, McnSegTable tb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const long long pid = a.pix[i];
    float d = 0.f;
    if (pid >= 0 && pid < a.npix) {                          // (an id outside the image: nothing is read)
        const int cam = mcn_segment_of_ray(tb, i).cam;
        const float v = a.depth[(size_t)cam * (size_t)a.npix + (size_t)pid];
        d = depth_valid(v) ? v : 0.f;
    }
    a.out[i] = d;
}

hipError_t mcn_launch_gather_depth(const McnGatherDepthArgs& a, const McnSegTable& t, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_depth_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a, t);
    return hipGetLastError();
}

// The depth term in two launches.  The first (train_loss_kernel's protocol, camera.hip): every block writes its partial of the squared
// error to out[4 + block] and its count of valid rays to out[4 + BLOCKS + block] (an integer word); the block that arrives last
// (counter in out[3], zero on entry, zero again on exit) adds both IN BLOCK ORDER and writes out[0..2] = (weight m, m, n_valid).
// s(a) - s(b) = (a - b) z_scale: the near plane cancels.
__global__ __launch_bounds__(256) void depth_loss_value_kernel(McnDepthLossArgs a) {
    __shared__ double red[256];
    __shared__ int cnt[256];
    __shared__ int last;
    const int t = threadIdx.x;
    double ar = 0.0;
    int nv = 0;
    for (int i = blockIdx.x * 256 + t; i < a.n; i += gridDim.x * 256) {
        const float d = a.d_gt[i];
        if (!depth_valid(d)) continue;
        ++nv;
        const float ec = (a.zexp_c[i] - d) * a.z_scale;
        ar += (double)ec * (double)ec;
        if (a.zexp_f) { const float ef = (a.zexp_f[i] - d) * a.z_scale; ar += (double)ef * (double)ef; }
    }
    red[t] = ar; cnt[t] = nv;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { red[t] += red[t + s]; cnt[t] += cnt[t + s]; }
        __syncthreads();
    }
    unsigned* words = reinterpret_cast<unsigned*>(a.out);
    if (t == 0) {
        a.out[4 + blockIdx.x] = (float)red[0];
        words[4 + MCN_DEPTH_LOSS_BLOCKS + blockIdx.x] = (unsigned)cnt[0];
        __threadfence();
        last = atomicAdd(words + 3, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last || t != 0) return;
    __threadfence();
    double sum = 0.0;
    unsigned nvalid = 0;
    for (int b = 0; b < (int)gridDim.x; ++b) {               // (block order: deterministic)
        sum += (double)__builtin_nontemporal_load(a.out + 4 + b);
        nvalid += __builtin_nontemporal_load(words + 4 + MCN_DEPTH_LOSS_BLOCKS + b);
    }
    const float m = (float)(sum / (double)(nvalid > 0 ? nvalid : 1u));
    a.out[0] = a.weight * m; a.out[1] = m; a.out[2] = (float)nvalid;
    words[3] = 0u;
}

// The second: the gradients (2 weight z_scale / n_valid) (s_pred - s_gt) of the valid rays, exactly 0 of the others; n_valid from out[2].
__global__ __launch_bounds__(256) void depth_loss_grad_kernel(McnDepthLossArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const float nv = a.out[2];
    const float gr = 2.f * a.weight * a.z_scale / (nv > 0.f ? nv : 1.f);
    const float d = a.d_gt[i];
    const bool ok = depth_valid(d);
    a.d_c[i] = ok ? gr * ((a.zexp_c[i] - d) * a.z_scale) : 0.f;
    if (a.zexp_f) a.d_f[i] = ok ? gr * ((a.zexp_f[i] - d) * a.z_scale) : 0.f;
}

hipError_t mcn_launch_depth_loss(const McnDepthLossArgs& a, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    int blocks = (a.n + 1023) / 1024;
    if (blocks > MCN_DEPTH_LOSS_BLOCKS) blocks = MCN_DEPTH_LOSS_BLOCKS;
    hipLaunchKernelGGL(depth_loss_value_kernel, dim3(blocks), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(depth_loss_grad_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}
