// Launcher interface of the error-guided pixel sampler (errmap.hip) between the C ABI (api.hip) and its kernels.  A header of its
// own for the reason mcnerf_multicam.h is one: mcnerf_kernels.h is part of the digest that ties the recorded MLP-kernel traffic
// (profiles/pmc_traffic_*.json) to the sources.
#pragma once
#include "mcnerf_multicam.h"

// the map's geometry: err [C, Th, Tw] over C images of H x W pixels in tiles of `tile` x `tile` (edge tiles are smaller)
struct McnErrGeom {
    int C, H, W, tile;
    int Th, Tw, T;            // ceil(H / tile), ceil(W / tile), Th * Tw
};
static inline McnErrGeom mcn_err_geom(int C, int H, int W, int tile) {
    McnErrGeom g = {C, H, W, tile, (H + tile - 1) / tile, (W + tile - 1) / tile, 0};
    g.T = g.Th * g.Tw;
    return g;
}
struct McnErrSampleArgs {
    const float* err;         // [C,Th,Tw]
    McnErrGeom g;
    float uniform_frac;       // the first (int)(uniform_frac * n_k) rays of segment k are uniform over the image
    const float* u;           // [n,2] uniforms
    int n;
    unsigned long long* cdf;  // [K,T] workspace: inclusive prefix sums of the integer tile weights of segment k's camera
    long long* pix;           // [n] out
};
hipError_t mcn_launch_errmap_sample(const McnErrSampleArgs& a, const McnSegTable& t, hipStream_t st);
struct McnErrUpdateArgs {
    float* err;               // [C,Th,Tw]
    unsigned int* scratch;    // [C,Th,Tw], all zero before and after
    McnErrGeom g;
    const long long* pix;     // [n]
    const float* rgb;         // [n,3]
    const float* gt;          // [n,3]
    int n;
    float beta, one_minus_beta;
};
hipError_t mcn_launch_errmap_update(const McnErrUpdateArgs& a, const McnSegTable& t, hipStream_t st);
