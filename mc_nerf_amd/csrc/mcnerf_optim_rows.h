// Row-lazy Rectified Adam (`"lazy_rows": True` param groups of RAdam): the launcher interface of optim_rows.hip, and the
// element update it shares with the dense kernel (optim.hip).
// A header of its own, as mcnerf_lens.h: mcnerf_kernels.h is part of the digest that ties the recorded MLP-kernel traffic to the sources.
//
// A tensor of such a group is R rows of L elements (its leading dimension indexes the rows).  A row is VISITED in a step when any element
// of its gradient row compares != 0.0f (-0.0 does not count, a denormal does); an unvisited row keeps the bits of its parameter, both
// moments and its step count.  A visited row advances its OWN step count t = row_step[r] + 1 and takes mcn_radam_element, the dense
// kernel's update, with `rectified` and `step_size` read from entry t - 1 of a device table [T,2] fp32 that the host fills
// from RAdam._rectification: (1.0 if N_sma >= 5 else 0.0, float32(step_size)).  t is clamped into [1, T] before the read.
#pragma once
#include "mcnerf_kernels.h"

// The Rectified-Adam update of element i (reference model/net_utils.py:62-63, 88-99); decay = wd * lr, ss = step_size * lr, the scalar
// step size / N_sma computed on the host exactly like the reference's 10-slot cache (:67-86):
//   v = beta2 v + (1-beta2) g^2 ;  m = beta1 m + (1-beta1) g
//   rectified (N_sma >= 5):    p -= wd*lr*p ;  p -= step_size*lr * m / (sqrt(v) + eps)
//   otherwise (step_size > 0): p -= wd*lr*p ;  p -= step_size*lr * m
// Every operation is rounded on its own (the build has -ffp-contract=off): both callers get the same bits from the same inputs.
__device__ __forceinline__ void mcn_radam_element(float* p, const float* g, float* m, float* v, long long i, float b1, float b2, float decay,
                                                  float ss, float eps, bool rectified, float step_size) {
    const float gi = g[i];
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    v[i] = vi; m[i] = mi;
    float pi = p[i];
    if (rectified) {
        pi += -decay * pi;
        pi += -ss * (mi / (sqrtf(vi) + eps));
    } else if (step_size > 0.f) {
        pi += -decay * pi;
        pi += -ss * mi;
    }
    p[i] = pi;
}

#define MCN_RADAM_ROWS_PER_BLOCK 4          // one wave per row, block 256

struct McnRadamRowsTable {                   // (travels by value in the kernel arguments: 3.4 KB)
    int n_tensors;
    int T;                                   // entries of `table`
    float lr, beta1, beta2, eps, wd;
    const float* table;                      // [T,2] (rectified, step_size) of step t at entry t - 1
    long long total_rows;                    // rows of all tensors of this launch
    float* p[MCN_RADAM_MAXT];
    const float* g[MCN_RADAM_MAXT];
    float* m[MCN_RADAM_MAXT];
    float* v[MCN_RADAM_MAXT];
    int* row_step[MCN_RADAM_MAXT];           // [R] per-row step counts
    long long row_len[MCN_RADAM_MAXT];       // L
    int first_row[MCN_RADAM_MAXT];           // prefix of the row counts: tensor i owns rows [first_row[i], first_row[i+1])
};
// guard as mcn_launch_radam's (may be null); count_skip: this launch counts a refused step in guard[1]
hipError_t mcn_launch_radam_rows(const McnRadamRowsTable& t, unsigned* guard, int count_skip, hipStream_t st);
