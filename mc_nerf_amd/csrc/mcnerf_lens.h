// Per-camera radial lens distortion of the training cameras (`lens_model` = "radial"): the device arithmetic of the
// undistortion, forward and backward, and the launcher interface of lens.hip.  The ray arithmetic around it is mcnerf_rays.h's, which
// calls these functions where its LENS option is on.  A header of its own, as mcnerf_multicam.h: mcnerf_kernels.h and
// mcnerf_common.h are part of the digest that ties the recorded MLP-kernel traffic to the sources.
//
// THE MODEL.  lens [C,2] = (k1, k2) per training camera, OpenCV's two-coefficient radial model with its meaning and sign.  With
// (x_u, y_u) the ideal normalised image coordinates and (x_d, y_d) the observed ones:
//     r_u^2 = x_u^2 + y_u^2,   D(r) = 1 + k1 r^2 + k2 r^4,   (x_d, y_d) = D(r_u) (x_u, y_u)            world -> pixel: closed form
// Pixel -> ray needs the inverse: a FIXED-COUNT safeguarded Newton iteration on the radius (no data-dependent exit: the wave stays
// uniform):
//     cam = Kinv [u + 1/2, v + 1/2, 1]^T          mcn_cam_of_pixel; x_d = cam[0], y_d = cam[1]
//     r_d = sqrtf(x_d^2 + y_d^2);  r <- r_d
//     8 times:  q = r^2;  f' = 1 + q (3 k1 + 5 k2 q);  r <- r - (r (1 + q (k1 + k2 q)) - r_d) / max(f', 0.25);  r <- min(max(r, 0), 2 r_d)
//     s = r_d > 0 ? r / r_d : 1;   cam <- (s x_d, s y_d, cam[2])        then mcn_ray_of_cam: rotate, subtract the origin, normalise
// The distortion acts on cam[0], cam[1]: the normalised image plane whenever Kinv's last row is (0, 0, 1).  At k1 = k2 = 0 r never
// moves and s = 1 exactly: the rays are the bits of the pinhole kernels.  The floor on f' and the clamp keep every output finite for
// any finite k; outside the region where r D(r) is monotone the result is defined by the iteration above and nothing more.
//
// BACKWARD.  The converged root is differentiated by the implicit function theorem, not through the iterations, with q = r^2 and
// f' (floored at 0.25 as above) of the final r.  (g_x, g_y) = the gradient arriving at (s x_d, s y_d), h = g_x x_d + g_y y_d:
//     ds/dk1 = -s q / f'      ds/dk2 = -s q^2 / f'      ds/d(x_d, y_d) = -s^3 (2 k1 + 4 k2 q) / f' (x_d, y_d)
//     d_lens[cam] += h (ds/dk1, ds/dk2)
//     gcam_d = (g_x s + h ds/dx_d,  g_y s + h ds/dy_d,  gcam[2])        -> d_kinv, the outer product with the pixel as before
//     dR uses the undistorted cam.                                          None of these divides by r_d.
#pragma once
#include "mcnerf_multicam.h"

#define MCN_LENS_NEWTON_STEPS 8

// The undistorted radius r of an observed radius rd (the iteration above).
__device__ __forceinline__ float mcn_lens_undistort_radius(float rd, float k1, float k2) {
    float r = rd;
#pragma unroll
    for (int it = 0; it < MCN_LENS_NEWTON_STEPS; ++it) {
        const float q = __fmul_rn(r, r);
        const float fp = __fadd_rn(1.f, __fmul_rn(q, __fadd_rn(__fmul_rn(3.f, k1), __fmul_rn(__fmul_rn(5.f, k2), q))));
        const float f = __fsub_rn(__fmul_rn(r, __fadd_rn(1.f, __fmul_rn(q, __fadd_rn(k1, __fmul_rn(k2, q))))), rd);
        r = __fsub_rn(r, f / fmaxf(fp, 0.25f));
        r = fminf(fmaxf(r, 0.f), __fmul_rn(2.f, rd));
    }
    return r;
}

// cam (x_d, y_d, z) -> (s x_d, s y_d, z) in place; hands back s and the final radius r.
__device__ __forceinline__ void mcn_lens_undistort_cam(float* cam, float k1, float k2, float* s_out, float* r_out) {
    const float rd = sqrtf(__fadd_rn(__fmul_rn(cam[0], cam[0]), __fmul_rn(cam[1], cam[1])));
    const float r = mcn_lens_undistort_radius(rd, k1, k2);
    const float s = rd > 0.f ? r / rd : 1.f;
    cam[0] = __fmul_rn(s, cam[0]);
    cam[1] = __fmul_rn(s, cam[1]);
    *s_out = s; *r_out = r;
}

// The implicit derivatives of s at the final radius r: ds[0] = ds/dk1, ds[1] = ds/dk2, ds[2] = the factor of (x_d, y_d) in ds/d(x_d, y_d).
__device__ __forceinline__ void mcn_lens_ds(float s, float r, float k1, float k2, float* ds) {
    const float q = r * r;
    const float fp = fmaxf(1.f + q * (3.f * k1 + (5.f * k2) * q), 0.25f);
    const float sf = s / fp;
    ds[0] = -(sf * q);
    ds[1] = -(sf * (q * q));
    ds[2] = -(sf * (s * s) * (2.f * k1 + (4.f * k2) * q));
}

// The backward of mcn_lens_undistort_cam at the observed point (xd, yd), with its s and r: d_k [2] += h (ds/dk1, ds/dk2), and gcam,
// the gradient arriving at the undistorted cam, becomes the gradient at the observed one (gcam[2] passes through).
__device__ __forceinline__ void mcn_lens_undistort_bwd(float xd, float yd, float s, float r, float k1, float k2, float* gcam, float* d_k) {
    float ds[3];
    mcn_lens_ds(s, r, k1, k2, ds);
    const float h = gcam[0] * xd + gcam[1] * yd;
    d_k[0] += h * ds[0];
    d_k[1] += h * ds[1];
    const float hx = h * ds[2];
    gcam[0] = gcam[0] * s + hx * xd;
    gcam[1] = gcam[1] * s + hx * yd;
}

struct McnLensRayBatchArgs {
    McnRayBatchArgs r;        // everything mcn_launch_ray_batch_fwd takes
    const float* lens;        // [C,2] (k1, k2)
};
hipError_t mcn_launch_lens_ray_batch_fwd(const McnLensRayBatchArgs& a, const McnSegTable& t, hipStream_t st);
struct McnLensRayBatchBwdArgs {
    McnRayBatchBwdArgs r;     // everything mcn_launch_ray_batch_bwd takes
    const float* lens;        // [C,2]
    float* d_lens;            // [C,2] accumulated (atomics)
};
hipError_t mcn_launch_lens_ray_batch_bwd(const McnLensRayBatchBwdArgs& a, const McnSegTable& t, hipStream_t st);
