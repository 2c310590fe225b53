// Row-lazy fused multi-tensor Rectified Adam for gfx950 (the rule is stated in mcnerf_optim_rows.h): the per-camera
// parameters of MC-NeRF are [C, L] tensors of which a one-camera step touches one row.  radam_kernel (optim.hip) decays the moments of
// every row on every step, moves rows along a stale first moment and bias-corrects them by the global step count; here every row is an
// optimiser of its own that steps only when its gradient row is not all zero.
//
// One wave per row, four rows per block.  The lanes stride over the row's L elements twice: once to vote whether the row is visited
// (a wave vote: the branch is wave-uniform), once to update it.  The wave owns the row, so nothing is atomic and the result does not
// depend on the order of anything.  The element arithmetic is mcn_radam_element, the function radam_kernel calls: a group whose
// rows are all visited on every step gets the bits of the dense kernel.
#include "mcnerf_optim_rows.h"

__global__ __launch_bounds__(256) void radam_rows_kernel(McnRadamRowsTable t, unsigned* guard, int count_skip) {
    if (guard && guard[0]) {
        if (count_skip && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&guard[1], 1u);
        return;
    }
    const long long row = (long long)blockIdx.x * MCN_RADAM_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= t.total_rows) return;                                  // (the whole wave)
    // wave -> (tensor, row): rows are dealt to tensors by their precomputed first-row index
    int ti = 0;
    while (ti + 1 < t.n_tensors && row >= t.first_row[ti + 1]) ++ti;
    const int r = (int)(row - t.first_row[ti]);
    const long long L = t.row_len[ti], base = (long long)r * L;
    const int lane = threadIdx.x & 63;
    const float* __restrict__ g = t.g[ti] + base;
    // visited: any element != 0.0f.  Tested on the bits, so that it does not depend on the denormal mode of the compare: everything but
    // +0.0 and -0.0 counts
    bool hit = false;
    for (long long i = lane; i < L; i += 64) hit |= (__float_as_uint(g[i]) & 0x7FFFFFFFu) != 0u;
    if (!__any(hit)) return;
    float* __restrict__ p = t.p[ti] + base;
    float* __restrict__ m = t.m[ti] + base;
    float* __restrict__ v = t.v[ti] + base;
    int* row_step = t.row_step[ti];
    const int step = row_step[r] + 1;
    const int e = (step < 1 ? 1 : step > t.T ? t.T : step) - 1;      // (the host keeps T >= step: the clamp never acts)
    const bool rectified = t.table[2 * e] != 0.f;
    const float step_size = t.table[2 * e + 1];
    const float b1 = t.beta1, b2 = t.beta2, decay = t.wd * t.lr, ss = step_size * t.lr;
    for (long long i = lane; i < L; i += 64) mcn_radam_element(p, g, m, v, i, b1, b2, decay, ss, t.eps, rectified, step_size);
    if (lane == 0) row_step[r] = step;
}

hipError_t mcn_launch_radam_rows(const McnRadamRowsTable& t, unsigned* guard, int count_skip, hipStream_t st) {
    const long long blocks = (t.total_rows + MCN_RADAM_ROWS_PER_BLOCK - 1) / MCN_RADAM_ROWS_PER_BLOCK;
    if (blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(radam_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, t, guard, count_skip);
    return hipGetLastError();
}
