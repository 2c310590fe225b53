// Alpha-mask supervision of the FRONT weight for gfx950 (the extension library; include/mcnerf_ext.h):
//   fg[n] = sum_{j + 1 < S} w_j,  w_j the rgb composite's weights of composite.hip -- every weight but the far-plane sample's, whose
//   delta = 1e10 takes whatever transmittance is left (sum_j w_j is 1 on every ray);
// the composite backward that takes a gradient on fg beside the one on rgb; the gather of the drawn pixels' alpha; the MSE term.
//
// front_weight_kernel is the fp64 weight sweep and composite_bwd_front_kernel the backward body of mcnerf_composite.h, which
// composite.hip and distortion.hip compile too: one wave per ray, grid-strided, the depths z = fl32(zrow[j] + jitter), a DPP
// inclusive product of u with a carry from chunk to chunk, the backward's two passes over LDS.  With d_fg null the backward is the
// core's instantiation and gives the bits of mcn_launch_composite_bwd, which tests/test_mask_ops_gpu.py asserts on every case.
// The reason for the sweep's fp64 is told there.
#include "mcnerf_mask.h"
#include "mcnerf_composite.h"

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
        float sg = 0.f, e1 = 0.f;
        if (j < S) { sg = sig[(size_t)j * 4]; e1 = a.eps[(size_t)n * S + j]; }
        const McnWeight64 q = mcn_weight_sweep64(sg, e1, zrow, jit, j, S, carryT);
        if (j + 1 < S) afg += q.w;                          // every sample but the far-plane one
    }
    afg = wave_last_f64(wave_incl_sum_f64(afg));
    if (lane == 0) a.fg[n] = (float)afg;
    }
}

hipError_t mcn_launch_front_weight(const McnFrontWeightArgs& a, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    hipLaunchKernelGGL(front_weight_kernel, dim3(min((a.N + 3) / 4, MCN_COMPOSITE_BLOCKS)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// The composite backward with a gradient on the front weight beside the one on rgb (mcnerf_composite.h); FRONT: d_fg is given.
template <bool FRONT>
__global__ __launch_bounds__(256) void composite_bwd_front_kernel(McnCompositeBwdFrontArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    mcn_composite_bwd_rays<FRONT, false>({a.sig_rgb, a.zgrid, a.jitter, a.eps, a.d_rgb, a.d_fg, nullptr, nullptr, 0.f, 0.f, a.N, a.S, a.white_back,
                                          a.d_sig_rgb, a.gmax_bits, a.z_stride}, sm);
}

hipError_t mcn_launch_composite_bwd_front(const McnCompositeBwdFrontArgs& a, hipStream_t st) {
    return mcn_launch_composite_bwd_rays(a.d_fg ? composite_bwd_front_kernel<true> : composite_bwd_front_kernel<false>, a, st);
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
