// The one 32-bit hash of the device-side random draws: keys of the random cap (select.hip), round function of the pixel permutation (mcnerf_rays.h).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned mcn_hash32(unsigned seed, unsigned i) {
    unsigned x = i * 0x9E3779B9u + seed;          // murmur3 finaliser: every output bit depends on every input bit
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
