// Wavefront (64-lane) scan / reduction helpers on the DPP path, shared by the one-wave-per-ray kernels (composite.hip,
// mcnerf_composite.h, sample_pdf.hip).  Every lane of the wave must be active where they are called.
#pragma once
#include "mcnerf_common.h"

// Wavefront scans on the DPP path (row shifts inside each 16-lane row, then row_bcast:15 / row_bcast:31 carry the row totals
// across: six full-rate vector ops with a DPP operand) instead of six ds_bpermute round trips through the LDS crossbar; lane 63 of
// an inclusive scan is the reduction (v_readlane).  A lane whose DPP source is out of range keeps `old` = the identity.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f(float ident, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(ident), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
#define MCN_WAVE_SCAN(OP, IDENT)                                                         \
    v = OP(v, dpp_f<0x111, 0xf>(IDENT, v));   /* row_shr:1 */                             \
    v = OP(v, dpp_f<0x112, 0xf>(IDENT, v));   /* row_shr:2 */                             \
    v = OP(v, dpp_f<0x114, 0xf>(IDENT, v));   /* row_shr:4 */                             \
    v = OP(v, dpp_f<0x118, 0xf>(IDENT, v));   /* row_shr:8 */                             \
    v = OP(v, dpp_f<0x142, 0xa>(IDENT, v));   /* row_bcast:15 into rows 1, 3 */           \
    v = OP(v, dpp_f<0x143, 0xc>(IDENT, v));   /* row_bcast:31 into rows 2, 3 */
__device__ __forceinline__ float op_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float op_add(float a, float b) { return a + b; }
__device__ __forceinline__ float wave_incl_prod(float v) { MCN_WAVE_SCAN(op_mul, 1.f) return v; }
__device__ __forceinline__ float wave_incl_sum(float v) { MCN_WAVE_SCAN(op_add, 0.f) return v; }
__device__ __forceinline__ float wave_shr1(float v, float ident) { return dpp_f<0x138, 0xf>(ident, v); }      // lane l <- lane l - 1, lane 0 <- ident (wave_shr:1)
__device__ __forceinline__ float wave_last(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
__device__ __forceinline__ float wave_sum(float v) { return wave_last(wave_incl_sum(v)); }
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_f<0x111, 0xf>(v, v)); v = fmaxf(v, dpp_f<0x112, 0xf>(v, v)); v = fmaxf(v, dpp_f<0x114, 0xf>(v, v));
    v = fmaxf(v, dpp_f<0x118, 0xf>(v, v)); v = fmaxf(v, dpp_f<0x142, 0xa>(v, v)); v = fmaxf(v, dpp_f<0x143, 0xc>(v, v));
    return wave_last(v);
}

// The same inclusive scan in fp64 (sample_pdf.hip: a CDF whose entries do not depend on the order of the sum): both 32-bit halves
// of a double take the same DPP moves; out-of-range lanes keep `ident` (0.0 for the sum, 1.0 for the product of the composite
// backward's fp64 transmittance, mcnerf_composite.h).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_d(double ident, double v) {
    const long long b = __double_as_longlong(v), o = __double_as_longlong(ident);
    const int lo = __builtin_amdgcn_update_dpp((int)o, (int)b, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double wave_incl_sum_f64(double v) {
    v += dpp_d<0x111, 0xf>(0.0, v); v += dpp_d<0x112, 0xf>(0.0, v); v += dpp_d<0x114, 0xf>(0.0, v); v += dpp_d<0x118, 0xf>(0.0, v);
    v += dpp_d<0x142, 0xa>(0.0, v); v += dpp_d<0x143, 0xc>(0.0, v);
    return v;
}
__device__ __forceinline__ double wave_incl_prod_f64(double v) {
    v *= dpp_d<0x111, 0xf>(1.0, v); v *= dpp_d<0x112, 0xf>(1.0, v); v *= dpp_d<0x114, 0xf>(1.0, v); v *= dpp_d<0x118, 0xf>(1.0, v);
    v *= dpp_d<0x142, 0xa>(1.0, v); v *= dpp_d<0x143, 0xc>(1.0, v);
    return v;
}
__device__ __forceinline__ double wave_shr1_f64(double v, double ident) { return dpp_d<0x138, 0xf>(ident, v); }
__device__ __forceinline__ double wave_last_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
