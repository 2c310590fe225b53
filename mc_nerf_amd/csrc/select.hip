// What the fine pass needs between the coarse weights and the fine MLP, entirely on the device:
// (1) Weight-threshold fine-sample selection (model/mc_nerf.py:623-629, 692-694, without the reference's host syncs .item(), nonzero): the
//     fine list's predicate over the shared compaction of mcnerf_compact.h, and the exclusive scan of every caller of it (voxel.hip too).
// (2) The random cap of the selected list (model/mc_nerf.py:630-632): cap_gather replays a given permutation, cap_random draws the
//     subset on the device.
// (3) The stand-alone positional encoding and its backward, and upload_f32 (small host values as kernel arguments).
#include "mcnerf_compact.h"
#include "mcnerf_hash.h"

// ------------------------------------------------------------------ selection
// min(weight_thresh, weights.max()) (model/mc_nerf.py:623)
__device__ __forceinline__ float sel_threshold(const McnSelectArgs& a) { return fminf(a.thresh, __uint_as_float(*a.wmax_bits)); }
struct SelectPred {             // (built behind the bounds check of the shared bodies: a wave beyond the batch does not read the word)
    const McnSelectArgs& a;
    const float thr;
    __device__ __forceinline__ SelectPred(const McnSelectArgs& a) : a(a), thr(sel_threshold(a)) {}
    __device__ __forceinline__ bool operator()(int n, int j) const { return a.w_sel[(size_t)n * a.Sc + j] >= thr; }
};
// The count and the write kernel of a list over [N, Sc] with `scale`, under any predicate on arguments that carry McnSelectArgs' names:
// the fine list below, and the hit library's lists (ray_skip.hip: the same predicate behind a ray's hit flag, and the flag alone).
template <typename Pred, typename Args>
__global__ __launch_bounds__(256) void select_count_kernel(Args a) {
    mcn_compact_count<Pred>(a.N, a.Sc, a.scale, a.sigma_default, a.ray_counts, a.out_f, a);
}

// Exclusive scan of ray_counts -> ray_offsets, total -> *count; the body is mcn_scan_counts (mcnerf_compact.h).  (The bounds and the hit
// library compile this file into themselves for it: ray_bounds.hip.)  One workgroup; N is at most ~1e6.  Every thread owns one contiguous run of `per` rays per thread: a private sum, ONE block-wide scan of the 1024 run sums, then the run's offsets -- two
// barriers in all.  A run is a multiple of four rays held in registers as int4 vectors: its loads (and its stores) are independent
// 16-byte operations in flight together (the scalar loop of dependent 4-byte loads over a 32-ray run took 53 us at 32768 rays);
// runs longer than 64 rays (N > 65536) or unaligned workspaces take the scalar loop.
__global__ __launch_bounds__(1024) void select_scan_kernel(McnSelectArgs a) {
    mcn_scan_counts(a.N, a.ray_counts, a.ray_offsets, a.count);
}

template <typename Pred, typename Args>
__global__ __launch_bounds__(256) void select_write_kernel(Args a) {
    mcn_compact_write<Pred>(a.N, a.Sc, a.scale, a.ray_offsets, a.idx, a);
}

hipError_t mcn_launch_select(const McnSelectArgs& a, hipStream_t st) {
    return mcn_launch_compact<McnSelectArgs, select_count_kernel<SelectPred, McnSelectArgs>, select_write_kernel<SelectPred, McnSelectArgs>>(a, st);
}
hipError_t mcn_launch_select_scan(int N, int* ray_counts, int* ray_offsets, int* count, hipStream_t st) {
    McnSelectArgs a = {};       // (the scan reads these four fields alone)
    a.N = N; a.ray_counts = ray_counts; a.ray_offsets = ray_offsets; a.count = count;
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError();
}

// Keeps idx_in[perm[i]], i < keep: the random cap of model/mc_nerf.py:630-632.
__global__ void cap_gather_kernel(const int2* idx_in, const long long* perm, int keep, int2* idx_out, int* count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < keep) idx_out[i] = idx_in[perm[i]];
    if (i == 0) *count = keep;
}
hipError_t mcn_launch_cap_gather(const int2* idx_in, const long long* perm, int keep, int2* idx_out, int* count, hipStream_t st) {
    if (keep <= 0) return hipSuccess;
    hipLaunchKernelGGL(cap_gather_kernel, dim3((keep + 255) / 256), dim3(256), 0, st, idx_in, perm, keep, idx_out, count);
    return hipGetLastError();
}

// ---- The random cap of model/mc_nerf.py:630-632 without a host round trip.  The reference keeps idx[randperm(K)[:keep]]
// when K > keep: a uniformly random subset of size `keep` (the order of the list never reaches a result).  Here every
// entry i < K gets a 32-bit key mcn_hash32(seed, i) and the `keep` smallest keys are kept: two 65536-bin histogram passes find
// the exact threshold key, a counting pass and an ordered compaction write the kept entries in list order.  K <= keep keeps everything.
// ws (uint32): [0 .. 65535] histogram of the high 16 key bits, [65536 .. 131071] histogram of the low 16 bits inside the
// boundary bin, [131072] boundary bin (0x10000 = keep all), [131073] entries below it, [131074] threshold key,
// [131075] ties to take at the threshold, [MCN_CAP_LT + b] / [MCN_CAP_EQ + b] entries of chunk b below / at the threshold.
__global__ __launch_bounds__(256) void cap_hist_hi_kernel(const int* count, int max_rows, int keep, const unsigned* seed, unsigned* ws) {
    const int K = min(*count, max_rows);
    if (K <= keep) return;
    const unsigned sd = *seed;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < K; i += gridDim.x * blockDim.x) atomicAdd(&ws[mcn_hash32(sd, i) >> 16], 1u);
}
// one workgroup: first bin whose inclusive prefix reaches `target`; writes (bin, prefix before it)
__device__ void cap_find(const unsigned* hist, unsigned target, unsigned* out_bin, unsigned* out_below) {
    __shared__ unsigned part[1024];
    const int tid = threadIdx.x;
    unsigned s = 0;
    for (int b = 0; b < 64; ++b) s += hist[tid * 64 + b];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned cum = 0;
        int t = 0;
        while (t < 1024 && cum + part[t] < target) { cum += part[t]; ++t; }
        int b = t * 64;
        if (t < 1024) { while (cum + hist[b] < target) { cum += hist[b]; ++b; } }
        *out_bin = (unsigned)b; *out_below = cum;
    }
    __syncthreads();
}
__global__ __launch_bounds__(1024) void cap_find_hi_kernel(const int* count, int max_rows, int keep, unsigned* ws) {
    const int K = min(*count, max_rows);
    if (K <= keep) { if (threadIdx.x == 0) { ws[131072] = 0x10000u; ws[131074] = 0xFFFFFFFFu; ws[131075] = 0xFFFFFFFFu; } return; }
    cap_find(ws, (unsigned)keep, &ws[131072], &ws[131073]);
}
__global__ __launch_bounds__(256) void cap_hist_lo_kernel(const int* count, int max_rows, int keep, const unsigned* seed, unsigned* ws) {
    const int K = min(*count, max_rows);
    if (K <= keep) return;
    const unsigned sd = *seed, bin = ws[131072];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < K; i += gridDim.x * blockDim.x) {
        const unsigned k = mcn_hash32(sd, i);
        if ((k >> 16) == bin) atomicAdd(&ws[65536 + (k & 0xFFFFu)], 1u);
    }
}
__global__ __launch_bounds__(1024) void cap_find_lo_kernel(const int* count, int max_rows, int keep, unsigned* ws) {
    const int K = min(*count, max_rows);
    if (K <= keep) return;
    __shared__ unsigned lo, below;
    cap_find(ws + 65536, (unsigned)keep - ws[131073], &lo, &below);
    if (threadIdx.x == 0) {
        ws[131074] = (ws[131072] << 16) | lo;                        // threshold key: all smaller keys are kept
        ws[131075] = (unsigned)keep - ws[131073] - below;            // ... and this many entries with exactly that key
    }
}
// The kept entries keep their order in the list (the reference's order whenever the cap does not bind, and a list that is the same,
// entry for entry, from run to run when it does: no atomic decides a position): every workgroup owns one contiguous chunk of
// the list, counts what it keeps (keys below the threshold, keys equal to it), and writes behind the chunks before it; of the entries
// whose key EQUALS the threshold the first `ties` in list order are taken.
__device__ __forceinline__ int cap_chunk(int K, int grid) { return (((K + grid - 1) / grid) + 255) & ~255; }
__global__ __launch_bounds__(256) void cap_count_kernel(const int* count, int max_rows, int keep, const unsigned* seed, unsigned* ws) {
    const int K = min(*count, max_rows);
    if (K <= keep) return;
    const unsigned sd = *seed, thr = ws[131074];
    const int chunk = cap_chunk(K, gridDim.x), lo = blockIdx.x * chunk, hi = min(K, lo + chunk);
    unsigned lt = 0, eq = 0;
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        const unsigned k = mcn_hash32(sd, (unsigned)i);
        lt += k < thr; eq += k == thr;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lt += __shfl_xor(lt, o); eq += __shfl_xor(eq, o); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&ws[MCN_CAP_LT + blockIdx.x], lt); atomicAdd(&ws[MCN_CAP_EQ + blockIdx.x], eq); }     // (integer sums: order-free)
}
// exclusive rank of `flag` among the 256 threads of the workgroup (in thread order) and the workgroup's total
__device__ __forceinline__ unsigned cap_block_rank(bool flag, unsigned* wsum, unsigned& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    __syncthreads();
    if (lane == 0) wsum[wv] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const unsigned v = wsum[w]; before += w < wv ? v : 0u; total += v; }
    return before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}
__global__ __launch_bounds__(256) void cap_write_kernel(const int2* idx_in, const int* count, int max_rows, int keep, const unsigned* seed,
                                                        unsigned* ws, int2* idx_out, int* count_out) {
    __shared__ unsigned wsum[4], red[8];
    const int K = min(*count, max_rows);
    if (blockIdx.x == 0 && threadIdx.x == 0) *count_out = min(K, keep);
    const int chunk = cap_chunk(K, gridDim.x), lo = blockIdx.x * chunk, hi = min(K, lo + chunk);
    if (K <= keep) {                                  // nothing to drop: the list as it stands
        for (int i = lo + threadIdx.x; i < hi; i += 256) idx_out[i] = idx_in[i];
        return;
    }
    const unsigned sd = *seed, thr = ws[131074], ties = ws[131075];
    unsigned lt = 0, eq = 0;                          // kept / tied entries of the chunks in front of this one
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) { lt += ws[MCN_CAP_LT + b]; eq += ws[MCN_CAP_EQ + b]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lt += __shfl_xor(lt, o); eq += __shfl_xor(eq, o); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = lt; red[4 + (threadIdx.x >> 6)] = eq; }
    __syncthreads();
    lt = red[0] + red[1] + red[2] + red[3];
    unsigned eq_run = red[4] + red[5] + red[6] + red[7];
    unsigned pos = lt + min(eq_run, ties);
    for (int base = lo; base < hi; base += 256) {
        const int i = base + threadIdx.x;
        const unsigned k = i < hi ? mcn_hash32(sd, (unsigned)i) : 0xFFFFFFFFu;
        const bool is_eq = i < hi && k == thr;
        unsigned n_eq, n_sel;
        const unsigned tie_rank = cap_block_rank(is_eq, wsum, n_eq);
        const bool sel = i < hi && (k < thr || (is_eq && eq_run + tie_rank < ties));
        const unsigned rank = cap_block_rank(sel, wsum, n_sel);
        if (sel) idx_out[pos + rank] = idx_in[i];
        pos += n_sel; eq_run += n_eq;
    }
}
hipError_t mcn_launch_cap_random(const int2* idx_in, const int* count, int max_rows, int keep, const unsigned* seed, unsigned* ws,
                                 int2* idx_out, int* count_out, hipStream_t st) {
    if (max_rows <= 0 || keep <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(ws, 0, MCN_CAP_WS * sizeof(unsigned), st);
    if (e != hipSuccess) return e;
    const int blocks = min((max_rows + 255) / 256, MCN_CAP_BLOCKS);
    hipLaunchKernelGGL(cap_hist_hi_kernel, dim3(blocks), dim3(256), 0, st, count, max_rows, keep, seed, ws);
    hipLaunchKernelGGL(cap_find_hi_kernel, dim3(1), dim3(1024), 0, st, count, max_rows, keep, ws);
    hipLaunchKernelGGL(cap_hist_lo_kernel, dim3(blocks), dim3(256), 0, st, count, max_rows, keep, seed, ws);
    hipLaunchKernelGGL(cap_find_lo_kernel, dim3(1), dim3(1024), 0, st, count, max_rows, keep, ws);
    hipLaunchKernelGGL(cap_count_kernel, dim3(blocks), dim3(256), 0, st, count, max_rows, keep, seed, ws);
    hipLaunchKernelGGL(cap_write_kernel, dim3(blocks), dim3(256), 0, st, idx_in, count, max_rows, keep, seed, ws, idx_out, count_out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ stand-alone positional encoding
// SinCosEmbedding.forward (model/net_block.py:20-35): [n,3] -> [n,3+6F] = [x, per axis sin(2^f x) f<F, cos(2^f x) f<F] (F = 10: 63)
// times the per-frequency BARF weights.  (The render path computes the same inside the fused MLP kernels.)
// (F = `emb_freqs_xyz` frequencies, 3 + 6 F output channels; one thread per (point, axis, frequency), F = 0: per (point, axis))
__global__ __launch_bounds__(256) void encode_kernel(const float* x, const float* barf_w, int n, int F, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int per = 3 * (F > 0 ? F : 1), nenc = 3 + 6 * F;
    if (i >= n * per) return;
    const int m = i / per, cf = i - m * per, c = F > 0 ? cf / F : cf, f = F > 0 ? cf - c * F : 0;
    const float xv = x[m * 3 + c];
    if (f == 0) out[(size_t)m * nenc + c] = xv;
    if (F == 0) return;
    float s, co;
    mcn_sincos(xv * (float)(1 << f), s, co);
    const float w = barf_w[f];
    out[(size_t)m * nenc + 3 + c * 2 * F + f] = s * w;
    out[(size_t)m * nenc + 3 + c * 2 * F + F + f] = co * w;
}
hipError_t mcn_launch_encode(const float* x, const float* barf_w, int n, int n_freqs, float* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int per = 3 * (n_freqs > 0 ? n_freqs : 1);
    hipLaunchKernelGGL(encode_kernel, dim3((n * per + 255) / 256), dim3(256), 0, st, x, barf_w, n, n_freqs, out);
    return hipGetLastError();
}
// its backward: d x_c = d out_c + sum_f w_f 2^f (cos(2^f x_c) d sin_f - sin(2^f x_c) d cos_f); one thread per (point, axis)
__global__ __launch_bounds__(256) void encode_bwd_kernel(const float* x, const float* barf_w, int n, int F, const float* d_out, float* d_x) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * 3) return;
    const int m = i / 3, c = i - m * 3;
    const float xv = x[i];
    const float* g = d_out + (size_t)m * (3 + 6 * F);
    float dx = g[c];
    for (int f = 0; f < F; ++f) {
        float s, co;
        mcn_sincos(xv * (float)(1 << f), s, co);
        dx = fmaf(barf_w[f] * (float)(1 << f), co * g[3 + c * 2 * F + f] - s * g[3 + c * 2 * F + F + f], dx);
    }
    d_x[i] = dx;
}
hipError_t mcn_launch_encode_bwd(const float* x, const float* barf_w, int n, int n_freqs, const float* d_out, float* d_x, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(encode_bwd_kernel, dim3((n * 3 + 255) / 256), dim3(256), 0, st, x, barf_w, n, n_freqs, d_out, d_x);
    return hipGetLastError();
}

// up to 16 host floats by value (kernel arguments) -> device memory: a stream-ordered upload that never blocks the host
struct McnFloats16 { float v[16]; };
__global__ void upload_f32_kernel(float* dst, McnFloats16 vals, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
}
hipError_t mcn_launch_upload_f32(float* dst, const float* host_vals, int n, hipStream_t st) {
    McnFloats16 v = {};
    for (int i = 0; i < n && i < 16; ++i) v.v[i] = host_vals[i];
    hipLaunchKernelGGL(upload_f32_kernel, dim3(1), dim3(64), 0, st, dst, v, n);
    return hipGetLastError();
}
