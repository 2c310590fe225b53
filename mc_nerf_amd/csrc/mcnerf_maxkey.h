// The deterministic "max per cell, single writer" update of a running fp32 map, defined once for the voxel sigma cache (voxel.hip) and
// the per-tile error map (errmap.hip).  Every item i of an update names a cell of the map and a value; item(i, cell, value) -> bool is
// false where there is nothing (beyond the list, outside the map, a non-finite value).  Two launches over the same items, whatever
// their order of arrival:
//   max     every item takes atomicMax of the order-preserving uint32 key of its value into scratch[cell] (0 = none: every finite
//           float's key is > 0);
//   blend   every item atomicExch'es scratch[cell] with 0, and the one thread that receives a non-zero key is the cell's single writer of
//             V <- (1 - beta) * V + beta * m      as  __fadd_rn(__fmul_rn(1 - beta, V), __fmul_rn(beta, m)),  1 - beta formed on the host.
// Untouched cells keep their bits, and scratch is all zero again afterwards.  One thread per item, workgroups of 256.
#pragma once
#include <hip/hip_runtime.h>

// order-preserving key of a float: a < b <=> key(a) < key(b); every finite float's key is > 0 (key(-FLT_MAX) = 0x00800000)
__device__ __forceinline__ unsigned vox_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float vox_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

template <typename Item>
__device__ __forceinline__ void mcn_cell_max(unsigned* scratch, Item item) {
    size_t cell; float v;
    if (!item((long long)blockIdx.x * 256 + threadIdx.x, cell, v)) return;
    atomicMax(&scratch[cell], vox_key(v));
}
template <typename Item>
__device__ __forceinline__ void mcn_cell_blend(float* map, unsigned* scratch, float beta, float one_minus_beta, Item item) {
    size_t cell; float v;
    if (!item((long long)blockIdx.x * 256 + threadIdx.x, cell, v)) return;
    const unsigned k = atomicExch(&scratch[cell], 0u);
    if (k == 0u) return;                                    // another item of this cell is its writer
    map[cell] = __fadd_rn(__fmul_rn(one_minus_beta, map[cell]), __fmul_rn(beta, vox_unkey(k)));
}
