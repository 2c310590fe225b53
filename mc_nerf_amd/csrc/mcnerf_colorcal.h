// Launcher interface of the colour-calibrated train loss (color_calib.hip) between the C ABI (api.hip) and its kernel.  A header of
// its own for the reason mcnerf_multicam.h is one: mcnerf_kernels.h is part of the digest that ties the recorded MLP-kernel traffic
// (profiles/pmc_traffic_*.json) to the sources.
#pragma once
#include "mcnerf_multicam.h"

#define MCN_CALIB_NPART 7           // partials of a block: squared error, sum gr e rgb per channel (gain), sum gr e per channel (bias)
#define MCN_CALIB_BLOCKS 128        // blocks of one launch at most: K segments x <= max(1, 128 / K) blocks each
// (include/mcnerf.h: MCNERF_TRAIN_LOSS_CALIB_WS = MCN_CALIB_BLOCKS * MCN_CALIB_NPART floats of `partials`)
struct McnTrainLossCalibArgs {
    const float* pd;          // [np,2] reprojected pixels (np may be 0)
    const float* ptg;         // [np,2]
    int np;
    float inv_w2, inv_h2;
    int normalise;
    const float* rgb_c;       // [n,3]
    const float* rgb_f;       // [n,3] or null
    const float* gt;          // [n,3]
    int n;                    // rays
    const float* color_w;     // [C,6]: gain - 1 (3), bias (3)
    int C;
    float reg_lambda;
    float* out;               // [0..3] = total, L_intr, L_rgb, L_reg; [4] = arrival counter (zero on entry and on exit)
    float* d_pd;              // [np,2]
    float* d_c;               // [n,3]
    float* d_f;               // [n,3] (with rgb_f)
    float* d_color;           // [C,6]
    float* partials;          // [segment][block][MCN_CALIB_NPART]
};
hipError_t mcn_launch_train_loss_calib(const McnTrainLossCalibArgs& a, const McnSegTable& t, hipStream_t st);
