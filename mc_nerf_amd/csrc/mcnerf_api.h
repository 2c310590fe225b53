// The preamble of a library's C ABI file (api.hip, ext_api.hip, reg_api.hip, geo_api.hip, box_api.hip, hit_api.hip, fit_api.hip): the error buffer behind
// <prefix>_last_error, the two status-returning reporters and the argument checks that more than one library makes.  Included by
// exactly ONE translation unit per library; everything here has internal linkage, so each .so keeps a thread-local buffer of its own
// and exports nothing but its header's names.  Host code only: no kernel source includes it, and it is no part of the MLP source digest.
#pragma once
#include "mcnerf_multicam.h"
#include <stdio.h>

static thread_local char g_err[512] = "";

static int fail(const char* where, const char* what) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, what);
    return -1;
}
static int check(const char* where, hipError_t e) {
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s: HIP error %d (%s)", where, (int)e, hipGetErrorString(e));
    return -2;
}
#define REQ(cond, name) do { if (!(cond)) return fail(name, "invalid argument: " #cond); } while (0)

// the depth layout of the sample-evaluating entry points: one grid (0) or one row per ray (S)
static bool z_ok(int z_stride, int S) { return z_stride == 0 || z_stride == S; }
// a float argument by value: no NaN and a magnitude of at most 3.0e38f (just below FLT_MAX; box_api.hip keeps a bound of its own)
static bool finite_f(float v) { return v == v && v >= -3.0e38f && v <= 3.0e38f; }

// The host-side segment table of a multi-camera ray batch, validated and copied into the by-value kernel argument.  Everything is
// checked before any HIP call (a bad table is refused on a machine without a GPU too).  max_seg: the longest segment allowed
// (H * W when the pixels are drawn without replacement, n otherwise; MCN_ANY_SEG where a segment has no bound of its own).
#define MCN_ANY_SEG (1ll << 32)
static int fill_segments(const char* name, McnSegTable& t, const int32_t* seg_cam, const int32_t* seg_start, int K, int C, int n, long long max_seg) {
    REQ(seg_cam && seg_start, name);
    REQ(K >= 1 && K <= MCN_MULTICAM_MAXSEG, name);
    REQ(C >= 1 && n >= 0 && n <= (1 << 29), name);
    REQ(seg_start[0] == 0 && seg_start[K] == n, name);
    t.K = K;
    for (int k = 0; k < K; ++k) {
        REQ(seg_cam[k] >= 0 && seg_cam[k] < C, name);
        REQ(seg_start[k + 1] >= seg_start[k], name);
        REQ((long long)seg_start[k + 1] - seg_start[k] <= max_seg, name);
        t.cam[k] = seg_cam[k]; t.start[k] = seg_start[k];
    }
    t.start[K] = n;
    return 0;
}
