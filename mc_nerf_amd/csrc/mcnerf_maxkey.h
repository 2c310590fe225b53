// The order-preserving uint32 key of a float that the deterministic "max per cell, single writer" updates share (voxel.hip: the voxel
// sigma cache; errmap.hip: the per-tile error map): atomicMax on the keys is a max on the floats, and 0 is free to mean "none".
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
