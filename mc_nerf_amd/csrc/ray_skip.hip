// Skipping the rays that miss the scene box (`ray_bounds_miss = "skip"`) for gfx950: the kernels of libmcnhit.so.
//
// In "aabb" mode (ray_bounds.hip) a ray that the box does not clip is still sampled on [near, far], at the full price of both MLPs.  The
// MLP kernels already run on a (ray, sample) list over the (sigma_default, 1, 1, 1) prefill, so not evaluating a ray is not listing it:
// this library builds the lists of both passes behind a per-ray flag, hit[n] = 1 iff ray n is CLIPPED (the rule: include/mcnerf_box.h).
//
// Nothing here restates device code.  ray_bounds.hip is compiled into this library as it stands (the library links none of another
// library's objects), and with it select.hip and voxel.hip: the flag is the one box_ray_span forms (ray_depths_kernel writes it beside
// the span, in its one launch), the lists are the shared ordered compaction (mcnerf_compact.h: count -> mcn_scan_counts -> write, no
// atomics, no LDS beyond the scan's) through the kernel pairs of select.hip and voxel.hip, under those files' own predicates behind the
// flag.  One wavefront owns one ray, so the flag is the same in every lane: it is read through readfirstlane and the branch on it is a
// scalar one -- the wave of a missed ray reads neither its weights nor the grid, and costs a hit ray's wave nothing.
#include "mcnerf_ray_skip.h"
#include "ray_bounds.hip"

// hit[n] != 0 of the wave's ray (n is the same in every lane of a wave: blockIdx.x * 4 + the wave's index in its workgroup)
__device__ __forceinline__ bool ray_is_hit(const int* hit, int n) { return __builtin_amdgcn_readfirstlane(hit[n]) != 0; }

// Inner{a}(n, j) of a ray with hit[n] != 0, false on every other ray; Args carries Inner's arguments (as its base) and `hit`
template <typename Inner, typename Args>
struct HitPred {
    const Args& a;
    const Inner inner;
    __device__ __forceinline__ HitPred(const Args& a) : a(a), inner{a} {}
    __device__ __forceinline__ bool operator()(int n, int j) const { return ray_is_hit(a.hit, n) && inner(n, j); }
};
// every sample of a ray with hit[n] != 0
struct HitRayPred {
    const McnListRaysArgs& a;
    __device__ __forceinline__ bool operator()(int n, int) const { return ray_is_hit(a.hit, n); }
};

hipError_t mcn_launch_list_rays(const McnListRaysArgs& a, hipStream_t st) {
    return mcn_launch_compact<McnListRaysArgs, select_count_kernel<HitRayPred, McnListRaysArgs>, select_write_kernel<HitRayPred, McnListRaysArgs>>(a, st);
}
using HitSelectPred = HitPred<SelectPred, McnHitSelectArgs>;
hipError_t mcn_launch_hit_select(const McnHitSelectArgs& a, hipStream_t st) {
    return mcn_launch_compact<McnHitSelectArgs, select_count_kernel<HitSelectPred, McnHitSelectArgs>, select_write_kernel<HitSelectPred, McnHitSelectArgs>>(a, st);
}
using HitVoxelPred = HitPred<VoxelPred, McnHitVoxelSelectArgs>;
hipError_t mcn_launch_hit_voxel_select(const McnHitVoxelSelectArgs& a, hipStream_t st) {
    return mcn_launch_compact<McnHitVoxelSelectArgs, voxel_count_kernel<HitVoxelPred, McnHitVoxelSelectArgs>, voxel_write_kernel<HitVoxelPred, McnHitVoxelSelectArgs>>(a, st);
}
