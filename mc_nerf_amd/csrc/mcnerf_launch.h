// Host launch layer shared by the MLP kernel translation units (mlp_*.hip, mlp16_*.hip, mlp_x3_*.hip): the launch rules that
// do not depend on the kernel.  Host code only.  A kernel file keeps what is specific to it: its shared-memory size, its threads
// per workgroup, its rows per pass and the choice of instantiation from the arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#pragma GCC visibility push(hidden)     // (one copy per library of the inline functions and their statics, none exported)

// compute units of the current device (256 if the query fails), asked once per process
inline int mcn_num_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        if (cus <= 0) cus = 256;
    }
    return cus;
}

// rows of a sample-evaluating launch: the capacity of the index list when there is one, every sample of every ray otherwise
template <class Args>
inline long long mcn_max_rows(const Args& a) { return a.count ? (long long)a.max_rows : (long long)a.n_rays * a.S; }

inline long long mcn_passes(long long rows, int rows_per_pass) { return (rows + rows_per_pass - 1) / rows_per_pass; }

// grid of a persistent kernel: one workgroup per pass (unit of work), at most one per compute unit
inline int mcn_persistent_grid(long long passes) {
    const int cus = mcn_num_cus();
    return (int)(passes < cus ? passes : cus);
}

// The one launch: nothing to do for an empty grid; the dynamic-LDS limit of the kernel is raised to what this launch asks for on
// every launch (no cache: an attribute belongs to a (kernel, device) pair, and setting it costs less than the launch).
template <class... Params, class... Args>
inline hipError_t mcn_launch(void (*kern)(Params...), long long grid, int threads, size_t lds_bytes, hipStream_t st, const Args&... args) {
    if (grid <= 0) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(threads), lds_bytes, st, args...);
    return hipGetLastError();
}

// f(std::integral_constant<int, W>) for the layer width W of the net: the widths the kernels are instantiated for
template <class F>
inline hipError_t mcn_for_width(int width, F&& f) {
    switch (width) {
        case 256: return f(std::integral_constant<int, 256>{});
        case 128: return f(std::integral_constant<int, 128>{});
        case 64:  return f(std::integral_constant<int, 64>{});
        case 32:  return f(std::integral_constant<int, 32>{});
    }
    return hipErrorInvalidValue;
}

#pragma GCC visibility pop
