/* mcnerf.h - C ABI of the MI355X-native MC-NeRF volumetric-rendering hot path (libmcnerf.so).
 *
 * The reference (SkylerGao/MC_NeRF) has NO plugin / FFI layer: its hot path is eager PyTorch inside
 * model/mc_nerf.py, model/net_block.py and model/net_utils.py.  The entry points below are therefore
 * this build's own boundary; each one names the reference code it replaces (file:line, relative to
 * the reference checkout).  The Python host classes in mc_nerf_amd/model mirror the reference's
 * MC_Model / NeRF_Model API and call these functions through ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch allocates inputs, outputs,
 *     gradients and workspaces); the library keeps no global state and frees nothing;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it, there
 *     are no host synchronisations and no internal streams;
 *   - return value: 0 = OK, negative = error; mcnerf_last_error() returns a thread-local message;
 *   - all floating point is fp32; sample index pairs are int32 (ray, sample); pixel ids int64;
 *   - a net is described by (depth, width, skip): `depth` trunk layers of `width` units with the
 *     encoded input re-concatenated ([x_enc, h]) at layer index `skip` (model/net_block.py:51-59);
 *     widths 32, 64, 128, 256 and depth <= 8 are built.  `skip`: -1 = none, 0 < skip < depth = that
 *     layer, skip >= 256 = the mask form: bits 8 + l set for every such layer l (bit 8 itself, layer 0,
 *     is ignored and may serve as the marker of the form) -- the reference's `skips` is a list
 *     (model/net_block.py:45, 55-58) -- and, when bit 7 is set, the SH degree of the colour head in
 *     bits 4..6 (`MLP_deg` 0 .. 3, model/net_block.py:43, 75-76; 3 (deg + 1)^2 sh.2 outputs; default 2), and in
 *     bits 0..3 the number of encoding frequencies + 1 (`emb_freqs_xyz` 0 .. 10, model/net_block.py:11-18:
 *     3 + 6 F encoded channels; 0 = the default 10).  The exact-fp32 entry points take any mask, degree and
 *     frequency count, the `_16` entry points (f16 / bf16 / f16x3 register chains) at most one skip layer and
 *     degrees 0 .. 2 (any frequency count: their kernels have the geometry of degree 2 and 10 frequencies; a smaller
 *     net's tensors are scattered into it by mcnerf_pack_weights_16 -- zero weights where it has no channel / row --
 *     and its weight gradients gathered back by mcnerf_mlp_dw_16; `barf_w` is always 10 values there);
 *   - parameters of one net live in ONE flat fp32 buffer in the reference's state-dict order
 *     (xyz_encoding_{1..depth}.0.{weight,bias}, sigma.0.*, sigma.2.*, sh.0.*, sh.2.*), Linear weights
 *     [out][in] row-major; gradients use the same layout.
 */
#ifndef MCNERF_H
#define MCNERF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MCNERF_ABI_VERSION 7      /* 7: per-ray depth rows (z_stride) and mcnerf_sample_pdf; 6: dtype 3 (f16x3h) of the register-chain entry points */
#define MCNERF_SKIP_MASK 256      /* `skip` >= this: the mask form of the conventions above */

/* Marks a pointer parameter that addresses HOST memory where its type alone does not say so (the segment tables, the values of
 * mcnerf_upload_f32); long long* and T* const* parameters are host arrays by their type.  Expands to nothing.  The Python binding is
 * derived from this header (mc_nerf_amd/_lib.py): it checks a tensor's dtype against a device pointer's element type and refuses a
 * tensor at a host position. */
#define MCNERF_HOST

int mcnerf_abi_version(void);
const char* mcnerf_last_error(void);

/* Sizes (in floats) of the flat parameter buffer and of the packed-weight buffer of one net, and the
 * number of samples one workgroup tile covers (workspace capacities need no rounding; informative). */
long long mcnerf_param_count(int depth, int width, int skip);
long long mcnerf_packed_count(int depth, int width, int skip);
int mcnerf_tile_rows(int width);
/* Float offsets of the 2*depth+8 tensors (reference state-dict order) inside the flat parameter
 * buffer; each tensor starts on a 16-byte boundary, so the buffer has a few padding floats. */
int mcnerf_param_offsets(int depth, int width, int skip, long long* offsets);

/* Re-lays the Linear weights into MFMA operand-fragment order (forward + transposed copies).
 * Must be called after every parameter update, before mlp_fwd / mlp_bwd.  No reference
 * counterpart (torch's addmm reads nn.Linear.weight directly, model/net_block.py:69-74). */
int mcnerf_pack_weights(int depth, int width, int skip, const float* params, float* packed, void* stream);

/* Ray generation for the selected pixels of ONE camera.
 * Replaces MC_Model.get_rays + generate_rand_rays (model/mc_nerf.py:124-145, 327-345):
 * pose [3,4] = world->cam [R|t], kinv [3,3], pix [n] = v*W+u  ->  rays_d [n,3] (unit), rays_o [n,3]. */
int mcnerf_raygen_fwd(const float* pose, const float* kinv, const int64_t* pix, int n, int W,
                      float* rays_d, float* rays_o, void* stream);
/* Backward of the above; ACCUMULATES into d_pose [3,4] and d_kinv [3,3] (caller zeroes them). */
int mcnerf_raygen_bwd(const float* pose, const float* kinv, const int64_t* pix, int n, int W,
                      const float* d_rays_d, const float* d_rays_o, float* d_pose, float* d_kinv, void* stream);

/* Fused sample generation + positional encoding + MLP + SH colour for one net.
 * Replaces the gather/encode/MLP/scatter part of NeRF_Model.inference (model/mc_nerf.py:688-701),
 * SinCosEmbedding.forward (model/net_block.py:20-35), CorseFine_NeRF.forward (model/net_block.py:67-78)
 * and eval_sh (model/net_utils.py:103-191).
 *   rays_o, rays_d [n_rays,3]; zgrid [S] = linspace(near,far,S); jitter [n_rays] or NULL;
 *   z_stride: 0 = every ray samples zgrid [S]; S = zgrid is [n_rays,S], one row of depths per ray (the dense fine pass of
 *        mcnerf_sample_pdf's z_all, with jitter NULL: its rows already hold it).  Sample j of ray r sits at
 *        zgrid[r * z_stride + j] + jitter[r] -- the only thing that ties these kernels to a shared grid.  The same argument,
 *        with the same meaning, is taken by mcnerf_mlp_bwd, the _16 entry points and both composites;
 *   barf_w [10] per-frequency mask (ones when BARF is off);
 *   idx  NULL  -> dense: every (ray, sample) of the [n_rays,S] grid is evaluated (coarse pass);
 *        !NULL -> [max_rows] int32 (ray, sample) pairs, *count of them valid (fine pass); workgroups
 *                 beyond *count exit, so no host sync is needed to size the launch;
 *   out  [n_rays,S,4] = (sigma_raw, r, g, b) written at (ray, sample); entries not listed in idx are
 *        left untouched (mcnerf_select_fine pre-fills the reference's defaults);
 *   act_save / enc_save / sh_save / mask_save: NULL for the no-grad path; otherwise workspaces of
 *        (depth+2)*capacity*width, capacity*64, capacity*32 floats and (depth+2)*capacity*width/32
 *        uint32 (1-bit ReLU masks) that receive what mcnerf_mlp_bwd / mcnerf_mlp_dw need
 *        (capacity >= number of evaluated samples). */
int mcnerf_mlp_fwd(int depth, int width, int skip, const float* params, const float* packed,
                   const float* rays_o, const float* rays_d, const float* zgrid, int z_stride, const float* jitter,
                   const float* barf_w, const int32_t* idx, const int32_t* count, int max_rows,
                   int n_rays, int S, float* out,
                   float* act_save, long long capacity, float* enc_save, float* sh_save, uint32_t* mask_save,
                   void* stream);

/* The two modules of model/net_block.py as stand-alone forward calls (exact fp32 MFMA; the render path never materialises
 * these tensors):
 *   mcnerf_encode   = SinCosEmbedding.forward (:20-35): x [n,3], barf_w [n_freqs] -> out [n, 3 + 6 n_freqs] (`emb_freqs_xyz`; 10 -> 63);
 *   mcnerf_mlp_apply = CorseFine_NeRF.forward (:67-78): x_enc [n,63], dirs [n,3] -> out [n,4] = (sigma_raw, r, g, b).
 * mcnerf_encode / mcnerf_encode_bwd accept n = 0 (nothing launched) and n_freqs = 0 (out = x; barf_w may then be NULL). */
int mcnerf_encode(const float* x, const float* barf_w, int n, int n_freqs, float* out, void* stream);

/* Stream-ordered upload of up to 16 host floats WITHOUT a host-device copy: the values travel as kernel arguments and a
 * one-wave kernel stores them to `dst` (device).  For the per-step host scalars of the train step (the ten BARF weights of
 * model/net_block.py:26-29, evaluated in fp32 on the host exactly as the reference does): a pageable hipMemcpy would block
 * the host until every kernel queued before it has finished, i.e. serialise host and device once per step. */
int mcnerf_upload_f32(float* dst, MCNERF_HOST const float* host_vals, int n, void* stream);
int mcnerf_mlp_apply(int depth, int width, int skip, const float* params, const float* packed, const float* x_enc,
                     const float* dirs, int n, float* out, void* stream);

/* The same two modules DIFFERENTIATED (both are autograd-differentiable in the reference; the host classes wrap these in
 * torch.autograd.Functions, model/net_block.py):
 *   mcnerf_encode_bwd:     d_out [n, 3 + 6 n_freqs] -> d_x [n,3] (written);
 *   mcnerf_mlp_apply_save: mcnerf_mlp_apply that also fills the exact-fp32 workspaces of mcnerf_mlp_fwd (capacity >= n);
 *   mcnerf_mlp_apply_bwd:  d_out [n,4] -> d_x_enc [n,63] (written), d_dirs [n,3] (ACCUMULATED: zero it first; the SH view-direction
 *                          term) and dy_save / dsh_save, from which mcnerf_mlp_dw reduces the parameter gradients as for the
 *                          render path.  `zero` is a device float holding 0 (the sample depth of the degenerate one-sample ray). */
int mcnerf_encode_bwd(const float* x, const float* barf_w, int n, int n_freqs, const float* d_out, float* d_x, void* stream);
int mcnerf_mlp_apply_save(int depth, int width, int skip, const float* params, const float* packed, const float* x_enc,
                          const float* dirs, int n, float* out, float* act_save, long long capacity, float* enc_save,
                          float* sh_save, uint32_t* mask_save, void* stream);
int mcnerf_mlp_apply_bwd(int depth, int width, int skip, const float* params, const float* packed, const float* dirs, const float* zero,
                         int n, const float* out, const float* d_out, const uint32_t* mask_save, long long capacity,
                         const float* enc_save, const float* sh_save, float* dy_save, float* dsh_save,
                         float* d_x_enc, float* d_dirs, void* stream);

/* Backward of mcnerf_mlp_fwd wrt the activations (the dX chain): consumes d_out [n_rays,S,4],
 * writes the pre-activation gradients of every layer to dy_save ((depth+2)*capacity*width floats) and
 * dsh_save (capacity*32: d sh.2 outputs in columns 0..26, d sigma_raw in column 27) and ACCUMULATES
 * d_rays_o / d_rays_d [n_rays,3] (through the sample positions, the encoding and the SH view
 * direction; either may be NULL).  All weight gradients come from mcnerf_mlp_dw.
 * Replaces autograd through model/net_block.py:22-33, 67-78 and model/mc_nerf.py:602, 635, 690-691. */
int mcnerf_mlp_bwd(int depth, int width, int skip, const float* params, const float* packed,
                   const float* rays_o, const float* rays_d, const float* zgrid, int z_stride, const float* jitter,
                   const float* barf_w, const int32_t* idx, const int32_t* count, int max_rows,
                   int n_rays, int S, const float* out, const float* d_out,
                   const uint32_t* mask_save, long long capacity, const float* enc_save, const float* sh_save,
                   float* dy_save, float* dsh_save, float* d_rays_o, float* d_rays_d, void* stream);

/* Weight / bias gradients of one net: dW_l = dY_l^T X_l, db_l = sum_rows dY_l, ACCUMULATED into
 * `grads` (flat, same layout as the parameters; caller zeroes it once per step).
 * `count` NULL -> `rows` rows are valid; otherwise *count (<= rows). */
int mcnerf_mlp_dw(int depth, int width, int skip, const int32_t* count, int rows,
                  const float* act_save, const float* enc_save, const float* dy_save, const float* dsh_save,
                  long long capacity, float* grads, void* stream);

/* ---- Register-chain modes (csrc/mcnerf_16.h, csrc/mcnerf_x3.h), selected by `dtype`:
 *   0 = f16, 1 = bf16: ONE v_mfma_f32_32x32x16_{f16|bf16} per product, fp32 accumulate, biases / epilogues / outputs in
 *       fp32, 2-byte saved operands.  Results agree with the fp32 path to the operand rounding of the dtype (f16: ~1e-5
 *       in rgb on the reference's fixtures), NOT in general to the 1e-4 parity bar.
 *   2 = f16x3: the fp32-GRADE mode.  Every operand is hi + lo (two f16, 22 significand bits), a product is three f16
 *       MFMAs into one fp32 accumulator (~2^-21 relative product error), saved operands are a hi and a lo plane
 *       (4 bytes per value).  This is the mode that meets the 1e-4 parity bar at 16-bit MFMA rates ON EVERY OUTPUT: colours /
 *       depth / opacity (measured 3e-7), ray gradients and every parameter gradient (<= 1e-4 of a tensor's largest entry on
 *       the reference's goldens, measured <= 1.2e-5).
 *   3 = f16x3h: the forward and the backward (dX) chains of dtype 2, instruction for instruction -- colours, selection and ray
 *       gradients are bit-identical to dtype 2's -- but only the HI plane of every saved operand is written (in dtype 0's
 *       workspace layout: 2 bytes per value), and mcnerf_mlp_dw_16 is dtype 0's single-pass f16 kernel on those planes
 *       (activations carry the chains' 2^3 scale): the weight-gradient operands are rounded to 11 significand bits, everything
 *       that reaches a colour or a dX stays at 22.  Packed weights and the sh.2-output workspace (which 4) as dtype 2, the
 *       other workspaces as dtype 0.
 *       GATE of this mode (ONE statement; DESIGN.md 2, README.md, smoke() and the tests say the same): rendered colours /
 *       depth / opacity, the selection list and the ray (camera) gradients meet dtype 2's 1e-4 bar -- they are dtype 2's
 *       bits.  The PARAMETER gradients do NOT: (i) against dtype 2's they are gated at 1e-3 of a tensor's largest entry
 *       (tests/test_model_gpu.py::test_f16x3h_runs_the_f16x3_chains; measured <= 6e-4: unbiased rounding of the dW operands to
 *       11 bits); (ii) against the fp32 oracle, over ALL 40 tensors, at the multiples of the reference's own reorder noise
 *       that dtype 2 is gated at -- worst tensor <= 4 x 1.7e-3, median tensor <= 40 x 2.2e-5 of a tensor's largest entry
 *       (__graft_entry__.PARITY_GATES; measured at 256 rays: 2.5e-3 / 9.8e-5, dtype 2: 2.4e-3 / 3.0e-5, exact fp32: 1.4e-3 / 1.6e-5).
 *       bench.py reports this mode as its headline with dtype 2's line beside it (`f16x3_value`) and every mode's measured
 *       gradient errors (`parity.gradient_parity`).
 * Same reference code replaced as the fp32 entry points above (model/net_block.py:20-35, 67-78;
 * model/net_utils.py:103-191; model/mc_nerf.py:688-701).
 * Packed weights are two fragment STREAMS (forward order, backward = transposed order); workspaces are
 * fragment-major and sized by mcnerf_ws_bytes_16 (capacity is rounded up to whole 256-row passes inside). */
long long mcnerf_packed_bytes_16(int depth, int width, int skip, int dtype, int backward);
/* range_flags (may be NULL): depth + 3 words, one per packed weight tensor in state-dict order (trunk layers 0 .. depth-1,
 * sigma.0, sh.0, sh.2); word t is OR-ed with 1 when tensor t holds a weight outside the mode's operand range (f16: |w| > 65504,
 * f16x3: |w| > 65504 / 2^8 = 255.9, any mode: not finite).  Sticky: zero the words once, read them when a step was refused. */
int mcnerf_pack_weights_16(int depth, int width, int skip, const float* params, void* packed_fwd, void* packed_bwd,
                           int dtype, uint32_t* range_flags, void* stream);
/* which: 0 = activations or pre-activation gradients (all depth+2 slots), 1 = encodings, 2 = ReLU bit masks (all slots),
 *        3 = d(sh.2 outputs / sigma_raw), 4 = sh.2 outputs */
long long mcnerf_ws_bytes_16(int depth, int width, int dtype, long long capacity, int which);
/* mcnerf_mlp_fwd in these modes.  act_ws / enc_ws / mask_ws / sh_ws: NULL (all four) for the no-grad path. */
int mcnerf_mlp_fwd_16(int depth, int width, int skip, int dtype, const float* params, const void* packed_fwd,
                      const float* rays_o, const float* rays_d, const float* zgrid, int z_stride, const float* jitter,
                      const float* barf_w, const int32_t* idx, const int32_t* count, int max_rows,
                      int n_rays, int S, float* out,
                      void* act_ws, long long capacity, void* enc_ws, uint32_t* mask_ws, void* sh_ws, void* stream);
/* mcnerf_mlp_bwd in these modes: dy_ws / dsh_ws receive 16-bit (f16x3: hi + lo) gradients scaled by the power of two derived from
 * *gmax_bits (f16 range); d_rays_o / d_rays_d are accumulated in fp32. */
int mcnerf_mlp_bwd_16(int depth, int width, int skip, int dtype, const float* params, const void* packed_bwd,
                      const float* rays_o, const float* rays_d, const float* zgrid, int z_stride, const float* jitter,
                      const float* barf_w, const int32_t* idx, const int32_t* count, int max_rows,
                      int n_rays, int S, const float* out, const float* d_out,
                      const uint32_t* mask_ws, long long capacity, const void* enc_ws, const void* sh_ws,
                      void* dy_ws, void* dsh_ws, float* d_rays_o, float* d_rays_d, const uint32_t* gmax_bits, void* stream);
/* mcnerf_mlp_dw in these modes (fp32 accumulation and fp32 float-atomic output into `grads`). */
int mcnerf_mlp_dw_16(int depth, int width, int skip, int dtype, const int32_t* count, int rows,
                     const void* act_ws, const void* enc_ws, const void* dy_ws, const void* dsh_ws,
                     long long capacity, float* grads, const uint32_t* gmax_bits, void* stream);

/* Alpha compositing of [N,S] samples per ray.
 * Replaces NeRF_Model.inference's compositing (model/mc_nerf.py:705-727) and sigma2weights
 * (model/mc_nerf.py:729-736); the N(0,1) draws of sigma2weights are explicit inputs.
 *   eps [N,S]: draw of the rgb composite; eps_sel [N,S] or NULL: draw of the selection weights
 *   (model/mc_nerf.py:619 / 662), which are written to w_sel [N,S] and max-reduced into *wmax_bits
 *   (float bits; caller zeroes it);  depth/opacity [N] may be NULL (training).
 *   zgrid [S] (z_stride 0) or [N,S] depth rows (z_stride S), as mcnerf_mlp_fwd: delta_j = z_{j+1} - z_j of the ray's own row. */
int mcnerf_composite_fwd(const float* sig_rgb, const float* rays_d, const float* zgrid, int z_stride, const float* jitter,
                         const float* eps, const float* eps_sel, int N, int S, int white_back,
                         float* rgb, float* depth, float* opacity, float* w_sel, uint32_t* wmax_bits, void* stream);
/* Backward of the rgb composite: d_rgb [N,3] -> d_sig_rgb [N,S,4].  gmax_bits (or NULL): max |d_sig_rgb| of the
 * launch as float bits, max-reduced into a caller-zeroed word (the gradient scale of mcnerf_mlp_bwd_16).
 * S <= 2048: a workgroup stages 5 floats per sample for each of its 4 rays in LDS, 160 KiB at S = 2048 (more is refused as an
 * invalid argument).  N = 0 is a no-op in both calls (the arrays may then be null pointers). */
int mcnerf_composite_bwd(const float* sig_rgb, const float* zgrid, int z_stride, const float* jitter, const float* eps,
                         const float* d_rgb, int N, int S, int white_back, float* d_sig_rgb, uint32_t* gmax_bits,
                         void* stream);

/* Weight-threshold fine-sample selection (model/mc_nerf.py:623-629): every coarse sample with
 * w_sel >= min(thresh, max w_sel) contributes `scale` fine samples (ray, j*scale + r), emitted in
 * torch.nonzero order into idx [N*Sc*scale] (int32 pairs) with the total in *count.  out_f
 * [N,Sc*scale,4] (or NULL) is pre-filled with (sigma_default, 1, 1, 1) (model/mc_nerf.py:692-694).
 * ray_counts / ray_offsets: int32 [N] workspaces. */
int mcnerf_select_fine(const float* w_sel, const uint32_t* wmax_bits, float thresh, int N, int Sc, int scale,
                       float sigma_default, int32_t* ray_counts, int32_t* ray_offsets,
                       int32_t* idx, int32_t* count, float* out_f, void* stream);
/* Inverse-CDF hierarchical sampling, the fine sampler of `fine_sampler = "pdf"` (a sys_param key of this build; the default,
 * "threshold", is the reference's weight-threshold refinement above, model/mc_nerf.py:613-632, which has no such sampler).
 * Vanilla NeRF's sample_pdf in a deterministic form, per ray n (csrc/sample_pdf.hip states it in full):
 *   zc = zgrid + jitter[n] (the coarse pass's depths, bit for bit; jitter NULL = 0), bin edges mid[i] = (zc[i] + zc[i+1]) / 2,
 *   pdf = (w[n, 1 .. Sc-2] + 1e-5) / sum, cdf = [0, cumsum(pdf)] (sum and running sums accumulated in fp64, each rounded once to
 *   fp32: independent of the summation order); each u[n,k] in [0,1] is inverted through the right-sided
 *   search ind = #{cdf <= u} with denom = pdf[ind-1] (the bin's OWN pdf entry, not a difference of CDF entries; < 1e-5 -> 1);
 *   z_all [N, Sc+I] = sort(zc ++ zs) ascending.  w [N,Sc] are the coarse selection weights (w_sel of mcnerf_composite_fwd),
 *   u [N,I] in any order.  3 <= Sc, 1 <= I, Sc + I <= 1024.  Not differentiated (z_all is a constant of the fine pass). */
#define MCNERF_PDF_MAX_SAMPLES 1024      /* bound on Sc + I */
int mcnerf_sample_pdf(const float* w, const float* zgrid, const float* jitter, const float* u, int N, int Sc, int I,
                      float* z_all, void* stream);

/* ---- Voxel sigma cache, the coarse sampler of `coarse_sampler = "voxel"` (a sys_param key of this build; the default, "dense",
 * evaluates the coarse net on the whole [N,Sc] grid as the reference does).  New symbols only: no existing entry point changes,
 * MCNERF_ABI_VERSION stays 7.  The reference sketches the cache and never allocates it: query_sigma / update_sigma
 * (model/mc_nerf.py:859-867) index a `sigma_voxels` grid that does not exist; these four entry points replace those two methods
 * and build the (ray, sample) list + prefill that inference(..., idx_render, coarse=True) (:682-704, prefill :689-694) consumes.
 *   vox [G,G,G] fp32: running raw (pre-softplus) coarse sigma per cell over the cube [bmin, bmax]^3; scratch [G,G,G] uint32, all
 *   zero between calls.  Both are caller-owned device buffers like every other pointer: nothing is allocated, nothing synchronises.
 *   2 <= G <= 1024;  s = float32(G) / float32(bmax - bmin), formed once by the caller in fp32 (there is no device division).
 *   Cell of a point p, per axis: i = (int) min(max((p - bmin) * s, 0), G - 1) (a NaN lands in cell 0; nothing indexes outside the
 *   grid), linear index (ix * G + iy) * G + iz.  Sample j of ray n sits at p = o + d * z, z = zgrid[j] + jitter[n] (jitter NULL = 0),
 *   every step a separately rounded fp32 multiply or add: the cell of a sample is a pure function of its inputs.
 *
 * mcnerf_voxel_select: every (ray, sample) pair with vox[cell] > thresh, in torch.nonzero (row-major) order, into idx [N*Sc] (int32
 * pairs) with the total in *count (0 is legal and leaves idx untouched); out_c [N,Sc,4] (or NULL) is pre-filled with
 * (sigma_default, 1, 1, 1).  ray_counts / ray_offsets: int32 [N] workspaces.  No atomic decides a position. */
#define MCNERF_VOXEL_MAX_G 1024      /* bound on G */
int mcnerf_voxel_select(const float* vox, int G, float bmin, float s, float thresh, const float* rays_o, const float* rays_d,
                        const float* zgrid, const float* jitter, int N, int Sc, float sigma_default, int32_t* ray_counts,
                        int32_t* ray_offsets, int32_t* idx, int32_t* count, float* out_c, void* stream);
/* The update rule, on the listed pairs idx[0 .. min(*count, max_rows)) (idx / count NULL: all N * Sc pairs) with the sigma of pair
 * (n, j) read from sig_rgb[n, j, 0] (sig_rgb [N,Sc,4], the coarse net's output): for each touched cell m = max of this call's
 * finite sigmas in it (non-finite ones are skipped), V <- (1 - beta) * V + beta * m evaluated as
 * fadd_rn(fmul_rn(one_minus_beta, V), fmul_rn(beta, m)) with one_minus_beta = float32(1) - float32(beta) formed by the caller.
 * Untouched cells keep their bits; the result does not depend on the order of arrival; scratch is all zero again afterwards. */
int mcnerf_voxel_update(float* vox, uint32_t* scratch, int G, float bmin, float s, float beta, float one_minus_beta,
                        const float* rays_o, const float* rays_d, const float* zgrid, const float* jitter, int N, int Sc,
                        const int32_t* idx, const int32_t* count, int max_rows, const float* sig_rgb, void* stream);
/* query_sigma (model/mc_nerf.py:859-862): out[i] = vox[cell(pts[i])], pts [M,3] -> out [M]. */
int mcnerf_voxel_query(const float* vox, int G, float bmin, float s, const float* pts, int M, float* out, void* stream);
/* update_sigma (model/mc_nerf.py:864-867): the update rule above on explicit points pts [M,3] with sigma [M]. */
int mcnerf_voxel_update_points(float* vox, uint32_t* scratch, int G, float bmin, float s, float beta, float one_minus_beta,
                               const float* pts, const float* sigma, int M, void* stream);

/* The random cap of model/mc_nerf.py:630-632: idx_out[i] = idx_in[perm[i]], i < keep; *count = keep. */
int mcnerf_cap_gather(const int32_t* idx_in, const int64_t* perm, int keep, int32_t* idx_out, int32_t* count, void* stream);

/* The same cap with the random subset drawn ON THE DEVICE (no host synchronisation): when *count > keep a uniformly
 * random subset of `keep` entries of idx_in[0 .. *count) is written to idx_out (order unspecified, as the order of the
 * list never reaches a result) and *count_out = keep; otherwise all *count entries are copied.  Entry i is ranked by a
 * 32-bit hash of (*seed, i); *seed is a device word (drawn from torch's device generator by the host classes).
 * ws: mcnerf_cap_ws_words() uint32 of scratch. */
long long mcnerf_cap_ws_words(void);
int mcnerf_cap_random(const int32_t* idx_in, const int32_t* count, int max_rows, int keep, const uint32_t* seed,
                      uint32_t* ws, int32_t* idx_out, int32_t* count_out, void* stream);

/* The pixel subset of a train step, randperm(H * W)[:batch] of model/mc_nerf.py:329, drawn on the device in one kernel:
 * out[i] = P(i), i < batch, with P a pseudo-random permutation of [0, n) keyed by the device word *seed (batch <= n <= 2^31):
 * distinct, uniformly distributed pixel ids in random order. */
int mcnerf_sample_perm(int64_t* out, long long n, int batch, const uint32_t* seed, void* stream);

/* Ground-truth colours of n pixels of ONE uint8 image resident in HBM:
 * image [H*W, channels] (channels 3 = RGB, 4 = RGBA composited on white as data/data_read.py:130-137),
 * pix [n] int64 -> out [n,3] fp32.  Replaces the per-step H2D image copy + gather (model/mc_nerf.py:379, 80). */
int mcnerf_gather_gt(const uint8_t* image, int channels, const int64_t* pix, int n, float* out, void* stream);

/* ---- The ray preamble of a MULTI-CAMERA train step (`cams_per_step` > 1, a sys_param key of this build; the default, 1, runs the
 * three single-camera entry points mcnerf_sample_perm / mcnerf_raygen_fwd / mcnerf_gather_gt as before).  New symbols only:
 * MCNERF_ABI_VERSION stays 7.  The reference has no such step (it ships one float image per step through its loader).
 *
 * A batch of n rays is K SEGMENTS of consecutive rays: segment k = rays [seg_start[k], seg_start[k+1]) of camera seg_cam[k].
 * seg_cam [K] and seg_start [K+1] are HOST arrays; the table is copied into the kernel arguments (no host-device copy, no host
 * synchronisation).  Refused (before any device work): K < 1, K > 64, a camera id outside [0, C), a decreasing seg_start,
 * seg_start[0] != 0, seg_start[K] != n, a segment longer than H * W when the pixels are drawn, channels not 3 or 4 with images.
 * A camera may be listed more than once, in any order.
 *
 * mcnerf_ray_batch_fwd: ONE launch for the whole preamble.  Replaces MC_Model.get_rays + generate_rand_rays and the ground-truth
 * gather (model/mc_nerf.py:124-145, 327-345, 379, 80) for a batch that spans cameras.  pose [C,3,4], kinv [C,3,3]; per ray i of
 * segment k:
 *   pixel  pix_in NULL: P_k(i - seg_start[k]), P_k the permutation of [0, H * W) of mcnerf_sample_perm keyed by
 *          *seed + k * 0x9E3779B9 (mod 2^32): segment 0 draws exactly what mcnerf_sample_perm draws from the same word, every
 *          segment's ids are distinct, two segments of one camera draw independently;  otherwise pix_in[i].  Written to pix_out [n];
 *   ray    rays_d / rays_o [n,3] from pose[seg_cam[k]], kinv[seg_cam[k]]: the bits of mcnerf_raygen_fwd for that camera and pixel;
 *   gt     images NULL: not written (gt may be NULL);  otherwise images [C, H*W, channels] uint8 -> gt [n,3], the bits of
 *          mcnerf_gather_gt on images[seg_cam[k]]. */
#define MCNERF_MULTICAM_MAXSEG 64      /* bound on K, here and in every other entry point that takes a segment table */
int mcnerf_ray_batch_fwd(const float* pose, const float* kinv, int C, MCNERF_HOST const int32_t* seg_cam, MCNERF_HOST const int32_t* seg_start, int K,
                         int n, int H, int W, const int64_t* pix_in, const uint32_t* seed, const uint8_t* images, int channels,
                         int64_t* pix_out, float* rays_d, float* rays_o, float* gt, void* stream);
/* Backward of the above (autograd through model/mc_nerf.py:124-145, 327-345): d_rays_d, d_rays_o [n,3] and the forward's pixels
 * pix [n] -> ACCUMULATES into d_pose [C,3,4] and d_kinv [C,3,3] (caller zeroes them: rows of cameras not in the table stay zero, a
 * camera listed in two segments receives the sum).  mcnerf_raygen_bwd's per-ray terms, summed in another order (float atomics). */
int mcnerf_ray_batch_bwd(const float* pose, const float* kinv, int C, MCNERF_HOST const int32_t* seg_cam, MCNERF_HOST const int32_t* seg_start, int K,
                         int n, int W, const int64_t* pix, const float* d_rays_d, const float* d_rays_o,
                         float* d_pose, float* d_kinv, void* stream);

/* ---- The same preamble with per-camera radial lens distortion (`lens_model` = "radial", a sys_param key of this build; the default,
 * "pinhole", runs the entry points above as before).  New symbols only: MCNERF_ABI_VERSION stays 7.  The reference has no lens model.
 *
 * lens [C,2] = (k1, k2) per training camera: OpenCV's two-coefficient radial model, (x_d, y_d) = (1 + k1 r^2 + k2 r^4) (x_u, y_u) with
 * r^2 = x_u^2 + y_u^2 on the normalised image plane.  A pixel's ray needs the inverse: cam = Kinv [u + 1/2, v + 1/2, 1]^T as
 * mcnerf_raygen_fwd forms it, (x_d, y_d) = cam[0..1], r_d = |(x_d, y_d)|, then eight safeguarded Newton steps on the radius from r = r_d,
 *   q = r^2;  f' = 1 + q (3 k1 + 5 k2 q);  r <- r - (r (1 + q (k1 + k2 q)) - r_d) / max(f', 0.25);  r <- min(max(r, 0), 2 r_d)
 * and cam <- (s x_d, s y_d, cam[2]), s = r / r_d (1 at r_d = 0), rotated and normalised as mcnerf_raygen_fwd does (csrc/mcnerf_lens.h
 * states the model in full).  Every output is finite for any finite k; at k = 0 every output has the bits of mcnerf_ray_batch_fwd.
 *
 * mcnerf_lens_ray_batch_fwd: mcnerf_ray_batch_fwd plus `lens`; ONE launch; pixels (the same draw from the same seed word) and ground
 *   truth exactly as mcnerf_ray_batch_fwd.  K = 1 is a one-segment table.
 * mcnerf_lens_ray_batch_bwd: mcnerf_ray_batch_bwd plus `lens` and d_lens [C,2]; ACCUMULATES into d_pose, d_kinv, d_lens (caller zeroes
 *   them).  The root is differentiated implicitly at the final radius, not through the iterations.
 * Both refuse, before any device work, everything mcnerf_ray_batch_fwd / _bwd refuse and a null lens / d_lens. */
int mcnerf_lens_ray_batch_fwd(const float* pose, const float* kinv, const float* lens, int C, MCNERF_HOST const int32_t* seg_cam, MCNERF_HOST const int32_t* seg_start,
                              int K, int n, int H, int W, const int64_t* pix_in, const uint32_t* seed, const uint8_t* images, int channels,
                              int64_t* pix_out, float* rays_d, float* rays_o, float* gt, void* stream);
int mcnerf_lens_ray_batch_bwd(const float* pose, const float* kinv, const float* lens, int C, MCNERF_HOST const int32_t* seg_cam, MCNERF_HOST const int32_t* seg_start,
                              int K, int n, int W, const int64_t* pix, const float* d_rays_d, const float* d_rays_o,
                              float* d_pose, float* d_kinv, float* d_lens, void* stream);

/* Fused camera parametrisation of all C cameras.
 * Replaces add_weights2intr / add_weights2pose / add_weights2calib_pose / se3_to_SE3 / taylor_A,B,C /
 * inverse_intrinsic (model/mc_nerf.py:171-210, 269-316) and the calibration reprojection branch get_reproject_pixels /
 * world2cam / cam2pix (model/mc_nerf.py:147-152, 236-267):
 *   K [C,3,3] = [[|W wfx|,0,|W/2 wux|],[0,|W wfy|,|H/2 wuy|],[0,0,1]], Kinv its analytic inverse,
 *   pose / calib [C,3,4] = se3_to_SE3(wpose / wpose_intr) with the reference's 11-term Taylor series,
 *   pix_intr [C,P,2] = pixels of wpts_intr [C,P,3] through (K, calib), pix_extr = wpts_extr through (K, pose)
 *   (each pair may be NULL: branch not evaluated).  C = 0 is accepted by both calls and launches nothing. */
int mcnerf_camera_fwd(const float* wpose, const float* wpose_intr, const float* wfx, const float* wfy, const float* wux,
                      const float* wuy, int C, int H, int W, float* K, float* Kinv, float* pose, float* calib,
                      const float* wpts_intr, const float* wpts_extr, int P, float* pix_intr, float* pix_extr, void* stream);
/* Backward of the above: upstream dK / dKinv [C,3,3], dpose / dcalib [C,3,4], dpix_intr / dpix_extr [C,P,2] (any may be
 * NULL) -> gradients of the six parameter tensors (WRITTEN, not accumulated). */
int mcnerf_camera_bwd(const float* wpose, const float* wpose_intr, const float* wfx, const float* wfy, const float* wux,
                      const float* wuy, int C, int H, int W, const float* dK, const float* dKinv, const float* dpose,
                      const float* dcalib, const float* wpts_intr, const float* wpts_extr, int P, const float* dpix_intr,
                      const float* dpix_extr, float* d_wpose, float* d_wpose_intr, float* d_wfx, float* d_wfy, float* d_wux,
                      float* d_wuy, void* stream);
/* Reprojection loss of n = B*C*P points (model/loss.py:45-58): *loss = mean((pd_x-gt_x)^2)/W^2 + mean((pd_y-gt_y)^2)/H^2;
 * backward: d_pd [n,2] from the device scalar *dloss. */
int mcnerf_reproj_loss_fwd(const float* pd, const float* gt, int n, int H, int W, float* loss, void* stream);
int mcnerf_reproj_loss_bwd(const float* pd, const float* gt, int n, int H, int W, const float* dloss, float* d_pd, void* stream);

/* The whole loss of a NeRF-stage train step, MC_NeRF_Loss.forward with the keys {"intr", "rgb"} (model/loss.py:13-31), value and
 * gradients in one launch:  total = L_intr / (L_intr + 1e-8) [normalise != 0: the GLOBAL_OPTIM / FINE_TUNE rescaling of :20-23, its
 * denominator a detached constant; normalise == 0: L_intr itself] + mean((rgb_c - gt)^2) + mean((rgb_f - gt)^2) [rgb_f may be null:
 * coarse only, :37-41].  pd, pt_gt [np,2] pixels (np may be 0), rgb_*, gt [nrgb] floats (nrgb = 3 N).
 * out[MCNERF_TRAIN_LOSS_OUT]: out[0..2] = {total, L_intr, rgb term}; out[3] is an arrival counter that must be ZERO on entry (it
 * is zero again on exit, so one zero-initialised buffer serves every call) and out[4..] per-block partial sums -- the value is
 * added in block order, i.e. deterministic;  d_pd [np,2], d_c, d_f [nrgb] = d total / d input.
 * mcnerf_scale3: a, b, c (c may be null) *= *g in place -- the saved gradients times the upstream gradient of the total. */
#define MCNERF_TRAIN_LOSS_OUT 132
int mcnerf_train_loss(const float* pd, const float* pt_gt, int np, int H, int W, int normalise,
                      const float* rgb_c, const float* rgb_f, const float* gt, int nrgb,
                      float* out, float* d_pd, float* d_c, float* d_f, void* stream);
int mcnerf_scale3(float* a, int na, float* b, int nb, float* c, int nc, const float* g, void* stream);

/* mcnerf_train_loss with a per-camera colour calibration (this build's own sys_param key "color_calib" = "affine"; it extends
 * MC_NeRF_Loss.forward for the keys {"intr", "rgb"}, model/loss.py:13-31, the reference has no colour correction): camera c is modelled
 * to observe g_c * rgb + b_c of the rendered colour, g_c = 1 + color_w[c, 0:3], b_c = color_w[c, 3:6], coarse and fine render alike.
 * The n rays are K segments of consecutive rays, segment k = rays [seg_start[k], seg_start[k+1]) of camera seg_cam[k] (HOST arrays, as
 * mcnerf_ray_batch_fwd's: they travel by value in the kernel arguments -- no host->device copy, no host synchronisation):
 *   L_rgb = mean_i,ch (g rgb_c[i] + b - gt[i])^2 + the same for rgb_f [may be null]      (g, b of the camera of ray i's segment)
 *   L_reg = reg_lambda * (1/K) sum_k mean_j color_w[c_k, j]^2                            (an empty segment adds nothing)
 *   total = the L_intr term exactly as mcnerf_train_loss (incl. the value-1 normalisation) + L_rgb + L_reg
 * Value and every gradient in ONE launch, deterministic (no float atomic decides a value): per ray and channel
 * e = (g rgb + b) - gt, evaluated in fp64 from the fp32 operands and rounded once (a small residual carries no cancellation error
 * into its camera's gradient row), and d rgb = (gr e) g with gr = 2 / (3 n), in that order, so that at color_w = 0 the residual
 * -- for colours in [0, 1] the correctly rounded rgb - gt -- and d_c / d_f are the bits of mcnerf_train_loss.  rgb_*, gt, d_c, d_f [n,3]; color_w, d_color [C,6] (rows of cameras outside the table
 * are exactly zero; a camera listed twice receives the sum of its segments);
 * out[MCNERF_TRAIN_LOSS_CALIB_OUT]: out[0..3] = {total, L_intr, L_rgb, L_reg}, out[4] an arrival counter that must be ZERO on entry
 * (it is zero again on exit); partials[MCNERF_TRAIN_LOSS_CALIB_WS] floats of scratch (seven partial sums per block, never read
 * before they are written: no initialisation needed).
 * Refused ahead of any device work: K < 1 or K > 64, a camera id outside [0, C), a decreasing seg_start, seg_start[0] != 0,
 * seg_start[K] != n, n < 1, reg_lambda < 0, a null required pointer. */
#define MCNERF_TRAIN_LOSS_CALIB_OUT 8
#define MCNERF_TRAIN_LOSS_CALIB_WS 896
int mcnerf_train_loss_calib(const float* pd, const float* pt_gt, int np, int H, int W, int normalise,
                            const float* rgb_c, const float* rgb_f, const float* gt, int n,
                            const float* color_w, int C, MCNERF_HOST const int32_t* seg_cam, MCNERF_HOST const int32_t* seg_start, int K, float reg_lambda,
                            float* out, float* d_pd, float* d_c, float* d_f, float* d_color, float* partials, void* stream);

/* ---- Error-guided pixel sampling (this build's own sys_param key "pixel_sampler" = "error"; the default, "uniform", runs
 * mcnerf_sample_perm / the in-kernel draw of mcnerf_ray_batch_fwd as before).  New symbols only: MCNERF_ABI_VERSION stays 7.  The
 * reference draws uniformly (model/mc_nerf.py:329).
 *
 * The map is err [C, Th, Tw] fp32, Th = ceil(H / tile), Tw = ceil(W / tile): a running squared colour error per tile of tile x tile
 * pixels of each of the C training images (edge tiles are smaller).  The n rays are K segments of consecutive rays, segment k = rays
 * [seg_start[k], seg_start[k+1]) of camera seg_cam[k]: HOST arrays that travel by value in the kernel arguments, as
 * mcnerf_ray_batch_fwd's (no host->device copy, no host synchronisation).
 *
 * Tile weights are integers, so the CDF does not depend on the order of summation:
 *   c_t = fminf(fmaxf(E_t, 0), 4) [NaN -> 0, +inf -> 4];  q_t = max(1, (uint64)(c_t * 2^24)) * area_t [area_t = pixels of tile t]
 * Pixel density is proportional to the clamped error; every tile keeps a non-zero weight; total <= 2^52 is exact in a double.
 *
 * mcnerf_errmap_sample: two launches (CDF: one block per segment writes the inclusive uint64 prefix sums of q of camera seg_cam[k]
 * into cdf[k][0 .. Th*Tw); draw: one thread per ray).  u [n,2] fp32 uniforms, both first clamped into [0, 1 - 2^-24] (NaN -> 0);
 * ray j of segment k (n_k rays), n_u = (int)((double)uniform_frac * n_k):
 *   j < n_u    pix = min((int64)((double)u0 * (double)(H W)), H W - 1)                                  (uniform over the image)
 *   otherwise  target = (uint64)((double)u0 * (double)total_k), tile t = the first with cdf[k][t] > target (clamped to Th*Tw - 1),
 *              l = min((int)(u1 * (float)area_t), area_t - 1) in fp32, pix = (ty tile + l / tw_t) W + tx tile + l % tw_t
 * -> pix [n] int64, every id in [0, H W) whatever the inputs.  Draws are WITH replacement.  cdf: a [>= K, Th*Tw] uint64 workspace.
 *
 * mcnerf_errmap_update: per ray d = rgb - gt, e = ((d0^2 + d1^2) + d2^2) * 0.333333343f, every step a separately rounded fp32
 * operation; rays with a non-finite e or pix outside [0, H W) are skipped.  Two launches, mcnerf_voxel_update's protocol: atomicMax
 * of the order-preserving key of e into scratch[seg_cam[k], tile(pix)]; then every ray exchanges its word with 0 and the one thread
 * that receives a non-zero key writes E <- fadd_rn(fmul_rn(one_minus_beta, E), fmul_rn(beta, m)) (one_minus_beta formed by the
 * caller in fp32).  Untouched tiles and cameras outside the table keep their bits; a camera listed in two segments gets the max over
 * both; deterministic whatever the order of arrival; scratch [C,Th,Tw] uint32 must be all zero on entry and is all zero on exit.
 *
 * Refused ahead of any device work: K < 1, K > 64, a camera id outside [0, C), a decreasing seg_start, seg_start[0] != 0,
 * seg_start[K] != n, tile < 1, H W > 2^26, uniform_frac (beta, one_minus_beta) outside [0, 1] or NaN, a null pointer. */
#define MCNERF_ERRMAP_MAX_PIXELS 67108864      /* bound on H W: 2^26 */
int mcnerf_errmap_sample(const float* err, int C, int H, int W, int tile, MCNERF_HOST const int32_t* seg_cam, MCNERF_HOST const int32_t* seg_start, int K,
                         int n, float uniform_frac, const float* u, uint64_t* cdf, int64_t* pix, void* stream);
int mcnerf_errmap_update(float* err, uint32_t* scratch, int C, int H, int W, int tile, MCNERF_HOST const int32_t* seg_cam, MCNERF_HOST const int32_t* seg_start,
                         int K, int n, const int64_t* pix, const float* rgb, const float* gt, float beta, float one_minus_beta,
                         void* stream);

/* Fused multi-tensor Rectified-Adam step (one launch for all tensors of a param group).
 * Replaces the per-tensor loop of RAdam.step (model/net_utils.py:38-99).  The arrays of n_tensors device
 * pointers / sizes live on the HOST; step_size and `rectified` (N_sma >= 5) are the host-side scalars of the
 * reference's step-size cache (model/net_utils.py:67-86) for the tensors' common step count.
 * guard (device uint32[2], or NULL): overflow guard of the reduced-precision modes -- guard[0] is raised when a gradient is
 * inf / NaN, an update then leaves parameters and moments untouched, and guard[1] counts refused steps (the caller
 * zero-initialises guard[1] once and reads it whenever it likes; no synchronisation here).
 * phase (bit set) lets ONE optimiser step that spans several calls (param groups, step counts) be refused as a whole:
 *   1 = clear guard[0] first, 2 = check this call's gradients, 4 = update this call's tensors, 8 = this call is the step's
 *   last update: count a refused step in guard[1].  A self-contained step is phase 15; a multi-call step runs (1|2), 2, ...
 *   over all its calls and then 4, ..., (4|8).  Within a call every check precedes every update. */
int mcnerf_radam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, const long long* sizes, float lr, float beta1, float beta2, float eps,
                      float weight_decay, float step_size, int rectified, uint32_t* guard, int phase, void* stream);

/* Row-lazy Rectified Adam (`"lazy_rows": True` param groups of RAdam): tensor i is n_rows[i] rows of row_len[i]
 * elements, and every row is an optimiser of its own that steps only when it is visited.  One launch per 64 tensors, one wave per row.
 *   visited    any element of the gradient row compares != 0.0f (-0.0 does not count, a denormal does)
 *   unvisited  parameter, both moments and row_step[i][r] keep their bits
 *   visited    t = row_step[i][r] + 1 is stored back;  v = beta2 v + (1-beta2) g g;  m = beta1 m + (1-beta1) g;  then the update of
 *              mcnerf_radam_step, expression for expression, with (rectified, step_size) = table[min(max(t, 1), T) - 1]: `table` is a
 *              DEVICE array [T,2] fp32 whose entry t - 1 holds (1.0 if N_sma(t) >= 5 else 0.0, step_size(t)), filled by the host from the
 *              formula of the reference's step-size cache.  The caller keeps T >= every t, so the clamp never acts.
 * The arrays of n_tensors device pointers / sizes live on the HOST.  guard (device uint32[2], or NULL) as mcnerf_radam_step's: with
 * guard[0] raised nothing is touched (row_step included), and with count_skip the call's last launch adds 1 to guard[1].  A step that
 * spans dense and lazy groups checks every gradient first (mcnerf_radam_step phase 2 on the flat sizes n_rows * row_len) and updates
 * afterwards.  Deterministic: a wave owns its row, nothing is atomic.
 * Refused ahead of any device work: a null pointer (guard excepted), n_tensors < 0, n_rows < 1 (or > 2^24), row_len < 1, T < 1. */
int mcnerf_radam_rows_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                           float* const* exp_avg_sq, int32_t* const* row_step, const long long* n_rows, const long long* row_len,
                           float lr, float beta1, float beta2, float eps, float weight_decay, const float* table, int T,
                           uint32_t* guard, int count_skip, void* stream);

/* Finish of the data-parallel step's ONE gradient all-reduce (mc_nerf_amd/distributed.py; replaces the bucketed reducer of
 * DistributedDataParallel, /root/reference main.py:60-62): `arena` = [n_grad summed gradient floats | n_flags summed flags]
 * after the SUM all-reduce.  One launch divides the gradients by `world` (DDP's average) and adds 1 to *asym when some rank's
 * "produced a gradient" flags differ from this rank's `local_flags` (sum != world * local): once per call, however many flags
 * differ.  n_grad = 0 and n_flags = 0 are accepted (local_flags may then be NULL; with both, nothing is launched). */
int mcnerf_sync_finish(float* arena, long long n_grad, int n_flags, int world, const float* local_flags, int32_t* asym, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MCNERF_H */
