// Per-camera colour calibration fused into the loss of a NeRF-stage train step (the reference has no counterpart:
// it extends MC_NeRF_Loss.forward for the keys {"intr", "rgb"}, model/loss.py:13-31, the launch of train_loss_kernel in camera.hip).
// Camera c is modelled to observe  g_c * rgb + b_c  of the rendered colour, g_c = 1 + color_w[c, 0:3], b_c = color_w[c, 3:6]:
//   L_rgb = mean_i,ch (g_cam(i) rgb_c[i] + b_cam(i) - gt[i])^2 + the same for rgb_f        cam(i): the camera of ray i's segment
//   L_reg = lambda (1/K) sum_k mean_j color_w[c_k, j]^2                                     (non-empty segments of the step)
//   total = L_intr term (as train_loss_kernel, incl. the value-1 normalisation) + L_rgb + L_reg
// ONE launch gives the value and every gradient.  2-D grid, blockIdx.y = segment of the McnSegTable in the kernel arguments: a
// block grid-strides over the rays of its own segment, whose six calibration values are wave-uniform (scalar loads).  Per ray and
// channel  e = (g rgb + b) - gt  and  d rgb = (gr e) g  with gr = 2 / (3 n), in that order.  The residual is evaluated in fp64 from
// the fp32 operands (g = 1 + w exactly) and rounded ONCE: in fp32 the roundings of 1 + w, of the product and of the two sums are
// ~1e-7 absolute, which a small residual (a fitted pixel, |e| < 0.03) carries into its camera's gradient row as more than the
// 2e-6 that row is held to (measured 2.04e-6 at one ray per camera).  At g = 1, b = 0 and colours in [0, 1] (the difference is exact in fp64) it is the correctly rounded rgb - gt, so
// the residual and d_c / d_f are the bits of train_loss_kernel.  A block reduces seven partials (MCN_CALIB_NPART) and stores
// them at partials[segment][block][7]; the block that arrives last (counter in out[4], zero on entry, zero again on exit) adds the
// squared errors in (segment, block) order, zeroes d_color, adds each segment's six gradient sums and its regulariser term
// 2 lambda / (6 K) w into row c_k serially over k (a camera listed twice receives the sum), evaluates the reprojection term as
// train_loss_kernel does, and writes out[0..3] and d_pd.  No float atomic decides a value: the result is deterministic, and rows
// of cameras outside the table are exactly zero.
#include "mcnerf_colorcal.h"
#include "mcnerf_wave.h"

__global__ __launch_bounds__(256) void train_loss_calib_kernel(McnTrainLossCalibArgs a, McnSegTable tb) {
    __shared__ float red[256];
    __shared__ float wred[4][MCN_CALIB_NPART];
    __shared__ float seg[MCN_MULTICAM_MAXSEG][6];
    __shared__ float segreg[MCN_MULTICAM_MAXSEG];
    __shared__ int last;
    const int t = threadIdx.x, k = blockIdx.y, nb = gridDim.x;
    const float* __restrict__ w = a.color_w + (size_t)tb.cam[k] * 6;
    const float g[3] = {1.f + w[0], 1.f + w[1], 1.f + w[2]};
    const double gd[3] = {1.0 + (double)w[0], 1.0 + (double)w[1], 1.0 + (double)w[2]}, bd[3] = {(double)w[3], (double)w[4], (double)w[5]};
    const float gr = 2.f / (float)(3 * a.n);
    float acc[MCN_CALIB_NPART];
#pragma unroll
    for (int j = 0; j < MCN_CALIB_NPART; ++j) acc[j] = 0.f;
    const int r1 = tb.start[k + 1];
    for (int r = tb.start[k] + blockIdx.x * 256 + t; r < r1; r += nb * 256) {
        const size_t o = (size_t)r * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float gv = a.gt[o + ch], c = a.rgb_c[o + ch];
            const float ec = (float)((gd[ch] * (double)c + bd[ch]) - (double)gv), dc = gr * ec;
            acc[0] += ec * ec;
            a.d_c[o + ch] = dc * g[ch];
            acc[1 + ch] += dc * c;
            acc[4 + ch] += dc;
            if (a.rgb_f) {
                const float f = a.rgb_f[o + ch];
                const float ef = (float)((gd[ch] * (double)f + bd[ch]) - (double)gv), df = gr * ef;
                acc[0] += ef * ef;
                a.d_f[o + ch] = df * g[ch];
                acc[1 + ch] += df * f;
                acc[4 + ch] += df;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MCN_CALIB_NPART; ++j) {
        const float s = wave_sum(acc[j]);
        if ((t & 63) == 0) wred[t >> 6][j] = s;
    }
    __syncthreads();
    if (t == 0) {
        float* p = a.partials + ((size_t)k * nb + blockIdx.x) * MCN_CALIB_NPART;
#pragma unroll
        for (int j = 0; j < MCN_CALIB_NPART; ++j) p[j] = ((wred[0][j] + wred[1][j]) + wred[2][j]) + wred[3][j];
        __threadfence();
        last = atomicAdd(reinterpret_cast<unsigned*>(a.out + 4), 1u) == (unsigned)(nb * gridDim.y) - 1u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    // ---- the last block: the reprojection term (train_loss_kernel's reduction, add for add)
    float ai = 0.f;
    for (int i = t; i < a.np; i += 256) {
        const float ex = a.pd[2 * i] - a.ptg[2 * i], ey = a.pd[2 * i + 1] - a.ptg[2 * i + 1];
        ai += ex * ex * a.inv_w2 + ey * ey * a.inv_h2;
    }
    red[t] = ai;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    // ---- per segment: its six gradient sums in block order, and its share of the regulariser
    const int K = tb.K;
    for (int i = t; i < K * 6; i += 256) {
        const int kk = i / 6, j = i - kk * 6;
        const float* p = a.partials + (size_t)kk * nb * MCN_CALIB_NPART + 1 + j;
        float s = 0.f;
        for (int bl = 0; bl < nb; ++bl) s += __builtin_nontemporal_load(p + (size_t)bl * MCN_CALIB_NPART);
        seg[kk][j] = s;
    }
    for (int kk = t; kk < K; kk += 256) {
        float s = 0.f;
        if (tb.start[kk + 1] > tb.start[kk]) {          // (an empty segment adds nothing)
            const float* wk = a.color_w + (size_t)tb.cam[kk] * 6;
            for (int j = 0; j < 6; ++j) s += wk[j] * wk[j];
        }
        segreg[kk] = s / 6.f;
    }
    for (int i = t; i < a.C * 6; i += 256) a.d_color[i] = 0.f;
    float sum = 0.f;
    for (int i = 0; i < K * nb; ++i) sum += __builtin_nontemporal_load(a.partials + (size_t)i * MCN_CALIB_NPART);      // ((segment, block) order)
    __syncthreads();
    float sreg = 0.f;
    for (int kk = 0; kk < K; ++kk) sreg += segreg[kk];
    const float regc = 2.f * a.reg_lambda / (6.f * (float)K);
    // row c = the sum over the segments k of camera c, serially over k: the thread of a camera's FIRST segment writes the row
    for (int i = t; i < K * 6; i += 256) {
        const int kk = i / 6, j = i - kk * 6, c = tb.cam[kk];
        bool first = true;
        for (int k2 = 0; k2 < kk; ++k2) first = first && tb.cam[k2] != c;
        if (!first) continue;
        const float wv = a.color_w[(size_t)c * 6 + j];
        float s = 0.f;
        for (int k2 = kk; k2 < K; ++k2)
            if (tb.cam[k2] == c && tb.start[k2 + 1] > tb.start[k2]) { s += seg[k2][j]; s += regc * wv; }
        a.d_color[(size_t)c * 6 + j] = s;
    }
    const float li = a.np > 0 ? red[0] / (float)a.np : 0.f, lr = sum / (float)(3 * a.n), lg = a.reg_lambda * sreg / (float)K;
    const float si = a.normalise ? 1.0f / (li + 1e-8f) : 1.0f;       // d total / d L_intr
    if (t == 0) {
        a.out[0] = (li * si + lr) + lg; a.out[1] = li; a.out[2] = lr; a.out[3] = lg;
        *reinterpret_cast<unsigned*>(a.out + 4) = 0u;
    }
    const float gi = si * 2.f / (float)(a.np > 0 ? a.np : 1);
    for (int i = t; i < a.np; i += 256) {
        a.d_pd[2 * i] = gi * (a.pd[2 * i] - a.ptg[2 * i]) * a.inv_w2;
        a.d_pd[2 * i + 1] = gi * (a.pd[2 * i + 1] - a.ptg[2 * i + 1]) * a.inv_h2;
    }
}

hipError_t mcn_launch_train_loss_calib(const McnTrainLossCalibArgs& a, const McnSegTable& t, hipStream_t st) {
    const int cap = MCN_CALIB_BLOCKS / t.K > 1 ? MCN_CALIB_BLOCKS / t.K : 1;       // K * blocks <= MCN_CALIB_BLOCKS (K <= 64)
    int blocks = (mcn_longest_segment(t) + 255) / 256;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(train_loss_calib_kernel, dim3(blocks, t.K), dim3(256), 0, st, a, t);
    return hipGetLastError();
}
