"""Tensor-level wrappers over the C ABI (include/mcnerf.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every function below
hands its tensors to ``_lib.call``, which checks them against the header's parameters (device, dtype,
contiguity) and passes raw pointers to libmcnerf.so, and returns tensors.  All launches go to
``torch.cuda.current_stream()``.  There is no CPU path.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _box, _ext, _fit, _geo, _hit, _lib, _reg

Tensor = torch.Tensor


# the limits and buffer sizes include/mcnerf.h defines
SKIP_MASK = _lib.DEFINES["MCNERF_SKIP_MASK"]                        # skip >= 256 = (bit mask of skip layers) << 8
MULTICAM_MAXSEG = _lib.DEFINES["MCNERF_MULTICAM_MAXSEG"]            # segments (cameras) of one step
PDF_MAX_SAMPLES = _lib.DEFINES["MCNERF_PDF_MAX_SAMPLES"]            # bound on Sc + n_importance of sample_pdf
VOXEL_MAX_G = _lib.DEFINES["MCNERF_VOXEL_MAX_G"]                    # cells per axis of the voxel sigma cache
ERRMAP_MAX_PIXELS = _lib.DEFINES["MCNERF_ERRMAP_MAX_PIXELS"]        # H * W of one image: the integer tile weights then sum to <= 2^52, exact in a double
TRAIN_LOSS_OUT = _lib.DEFINES["MCNERF_TRAIN_LOSS_OUT"]
TRAIN_LOSS_CALIB_OUT = _lib.DEFINES["MCNERF_TRAIN_LOSS_CALIB_OUT"]
TRAIN_LOSS_CALIB_WS = _lib.DEFINES["MCNERF_TRAIN_LOSS_CALIB_WS"]
# ... and include/mcnerf_ext.h, the extension library's header (`_ext`: loaded on the first call of one of its entry points)
MASK_LOSS_OUT = _ext.DEFINES["MCNERF_EXT_MASK_LOSS_OUT"]
# ... and include/mcnerf_reg.h, the regulariser library's (`_reg`: loaded on the first call of one of its entry points as well)
DIST_MOMENT_BYTES = _reg.DEFINES["MCNERF_REG_MOMENT_BYTES"]
# ... and include/mcnerf_geo.h, the geometry library's (`_geo`: loaded on the first call of one of its entry points too)
DEPTH_LOSS_OUT = _geo.DEFINES["MCNERF_GEO_DEPTH_LOSS_OUT"]


def skip_code(skips, depth: int, deg: int = 2, n_freqs: int = 10) -> int:
    """The reference's `skips` list, `MLP_deg` and `emb_freqs_xyz` (model/net_block.py:11-18, 43-45) -> the C ABI's `skip` argument:
    -1 (no skip layer), the layer index (one), or the mask form -- (bit mask of skip layers | 1) << 8, with 0x80 | deg << 4 in the low
    byte when the SH degree is not 2 and n_freqs + 1 in its low nibble when that is not 10 (several skip layers, another degree or
    frequency count: exact-fp32 kernels only)."""
    ks = sorted({int(k) for k in skips if 0 < int(k) < depth})
    if not 0 <= deg <= 3:
        raise ValueError("SH degrees 0 .. 3 are built")
    if not 1 <= n_freqs <= 10:
        raise ValueError("1 .. 10 encoding frequencies are built (64-column encoded-input tiles)")
    if deg == 2 and n_freqs == 10 and not ks:
        return -1
    if deg == 2 and n_freqs == 10 and len(ks) == 1:
        return ks[0]
    return ((sum(1 << k for k in ks) | 1) << 8) | ((0x80 | (deg << 4)) if deg != 2 else 0) | ((n_freqs + 1) if n_freqs != 10 else 0)


@dataclass(frozen=True)
class Net:
    """(depth, width, skip) of one CorseFine_NeRF (model/net_block.py:40-49 in the reference); `skip` in the C ABI's encoding
    (`skip_code`)."""
    depth: int
    width: int
    skip: int

    @property
    def triple(self):
        return (self.depth, self.width, self.skip)

    @property
    def skips(self):
        if self.skip >= SKIP_MASK:
            return [l for l in range(1, self.depth) if (self.skip >> 8) >> l & 1]
        return [self.skip] if 0 < self.skip < self.depth else []

    @property
    def multi_skip(self) -> bool:
        return len(self.skips) > 1

    @property
    def deg(self) -> int:
        return (self.skip >> 4) & 7 if self.skip >= SKIP_MASK and self.skip & 0x80 else 2

    @property
    def n_sh(self) -> int:
        return 3 * (self.deg + 1) ** 2

    @property
    def n_shp(self) -> int:
        return 32 if self.n_sh < 32 else 64

    @property
    def n_freqs(self) -> int:
        return (self.skip & 15) - 1 if self.skip >= SKIP_MASK and self.skip & 15 else 10

    @property
    def n_enc(self) -> int:
        return 3 + 6 * self.n_freqs

    @property
    def fp32_only(self) -> bool:
        """Topologies only the exact-fp32 kernel family takes: more than one skip layer, SH degree 3.  (The register-chain modes have
        the geometry of one skip layer, degree 2 and 10 frequencies; a net with fewer frequencies or a lower degree is scattered
        into it when its weights are packed, csrc/mcnerf_common.h.)"""
        return self.multi_skip or self.deg > 2

    def in_features(self, i: int) -> int:
        if i == 0:
            return self.n_enc
        return self.width + self.n_enc if i in self.skips else self.width

    def shapes(self):
        """Tensor shapes in the reference's state-dict order."""
        s = []
        for i in range(self.depth):
            s += [(self.width, self.in_features(i)), (self.width,)]
        s += [(self.width, self.width), (self.width,), (1, self.width), (1,),
              (self.width, self.width), (self.width,), (self.n_sh, self.width), (self.n_sh,)]
        return s

    def names(self):
        n = []
        for i in range(self.depth):
            n += [f"xyz_encoding_{i+1}.0.weight", f"xyz_encoding_{i+1}.0.bias"]
        n += ["sigma.0.weight", "sigma.0.bias", "sigma.2.weight", "sigma.2.bias",
              "sh.0.weight", "sh.0.bias", "sh.2.weight", "sh.2.bias"]
        return n


def param_count(net: Net) -> int:
    return int(_lib.lib().mcnerf_param_count(*net.triple))


def packed_count(net: Net) -> int:
    return int(_lib.lib().mcnerf_packed_count(*net.triple))


def param_offsets(net: Net):
    import ctypes
    n = 2 * net.depth + 8
    arr = (ctypes.c_longlong * n)()
    _lib.call("mcnerf_param_offsets", *net.triple, ctypes.cast(arr, ctypes.c_void_p))
    return [int(v) for v in arr]


def tile_rows(width: int) -> int:
    return int(_lib.lib().mcnerf_tile_rows(width))


# --------------------------------------------------------------------------- helpers
def _stream():
    # (before the runtime is up there is no device tensor: the null stream, and `_lib.call` refuses the host tensors it is handed)
    return torch.cuda.current_stream().cuda_stream if torch.cuda.is_initialized() else 0


def _depths(zgrid: Optional[Tensor], z_rows: Optional[Tensor], n_rays: int):
    """(depth tensor, S, z_stride) of the ops that evaluate samples: the shared grid `zgrid` [S] (z_stride 0: sample j of ray r at
    zgrid[j] + jitter[r]) or, when given, the per-ray depth rows `z_rows` [n_rays, S] (z_stride S: sample j of ray r at z_rows[r, j]
    + jitter[r]; `zgrid` is then not read)."""
    if z_rows is None:
        return zgrid, zgrid.numel(), 0
    if z_rows.dim() != 2 or z_rows.shape[0] != n_rays:
        raise _lib.McnerfError(f"z_rows must be [n_rays = {n_rays}, S], got {tuple(z_rows.shape)}")
    return z_rows, z_rows.shape[1], z_rows.shape[1]


def flatten_params(net: Net, tensors, device) -> Tensor:
    """Copies per-tensor parameters (reference order) into a fresh flat buffer."""
    flat = torch.zeros(param_count(net), dtype=torch.float32, device=device)
    for off, shp, t in zip(param_offsets(net), net.shapes(), tensors):
        n = 1
        for d in shp:
            n *= d
        flat[off:off + n].copy_(t.reshape(-1))
    return flat


# --------------------------------------------------------------------------- ops
PRECISIONS = ("f32", "f16x3", "f16x3h", "f16", "bf16")
# register-chain modes: single-pass 16-bit MFMA (csrc/mcnerf_16.h) and split-f16 "f16x3" (csrc/mcnerf_x3.h): name -> dtype
# code of the C ABI
# "f16x3h": the split-f16 forward / backward chains (colours and dX as in "f16x3") saving only the hi plane of every operand; the
# weight gradient is the single-pass f16 kernel on those planes (dW operands rounded to 11 bits; 2-byte saved operands)
DTYPE16 = {"f16": 0, "bf16": 1, "f16x3": 2, "f16x3h": 3}


def is16(precision: str) -> bool:
    return precision in DTYPE16


def packed16_split(net: Net, packed: Tensor, precision: str):
    """The register-chain modes keep both fragment streams of a net in ONE byte tensor: (forward stream, backward stream) views."""
    nf = int(_lib.lib().mcnerf_packed_bytes_16(*net.triple, DTYPE16[precision], 0))
    return packed[:nf], packed[nf:]


def pack_weights(net: Net, params: Tensor, packed=None, precision: str = "f32", range_flags: Optional[Tensor] = None):
    """Packed weights for the given precision mode: one fp32-sized buffer (f32: fp32 fragments, f16x3: split-f16
    fragments) or, in the 16-bit modes, one byte tensor holding the forward and the backward fragment stream.
    `range_flags` (int32 [depth + 3], 16-bit modes): sticky per-tensor "a weight is outside the mode's operand range" words
    (include/mcnerf.h: mcnerf_pack_weights_16)."""
    assert precision in PRECISIONS
    if is16(precision):
        if packed is None:
            l = _lib.lib()
            dt = DTYPE16[precision]
            packed = torch.empty(int(l.mcnerf_packed_bytes_16(*net.triple, dt, 0)) + int(l.mcnerf_packed_bytes_16(*net.triple, dt, 1)),
                                 dtype=torch.uint8, device=params.device)
        pf, pb = packed16_split(net, packed, precision)
        _lib.call("mcnerf_pack_weights_16", *net.triple, params, pf, pb, DTYPE16[precision],
                  range_flags, _stream())
        return packed
    if packed is None:
        packed = torch.empty(packed_count(net), dtype=torch.float32, device=params.device)
    _lib.call("mcnerf_pack_weights", *net.triple, params, packed, _stream())
    return packed


# ---- range watch of the reduced-precision modes: (flags tensor, owner label, tensor names, precision) per net that has packed weights
# with `range_flags`; read (one synchronisation) only when somebody asks why optimiser steps were refused
_RANGE_WATCH = []
RANGE_TEXT = {"f16": "|w| <= 65504", "bf16": "finite weights", "f16x3": "|w| <= 255.9 (the weights are scaled by 2^8 into f16)",
              "f16x3h": "|w| <= 255.9 (the weights are scaled by 2^8 into f16)"}


def range_watch_register(flags: Tensor, label: str, names, precision: str):
    import weakref
    _RANGE_WATCH[:] = [w for w in _RANGE_WATCH if w[0]() is not None]         # (models come and go: drop the words of dead ones)
    _RANGE_WATCH.append((weakref.ref(flags), label, list(names), precision))


def range_report():
    """[(label, tensor name, precision)] of every watched weight tensor that has held a value outside its mode's operand range."""
    out = []
    for ref, label, names, precision in list(_RANGE_WATCH):
        flags = ref()
        if flags is None:
            continue
        for i in torch.nonzero(flags.cpu()).reshape(-1).tolist():
            out.append((label, names[i], precision))
    return out


def raygen_fwd(pose: Tensor, kinv: Tensor, pix: Tensor, W: int) -> Tuple[Tensor, Tensor]:
    n = pix.numel()
    d = torch.empty(n, 3, dtype=torch.float32, device=pix.device)
    o = torch.empty_like(d)
    _lib.call("mcnerf_raygen_fwd", pose, kinv, pix, n, W, d, o, _stream())
    return d, o


def raygen_bwd(pose: Tensor, kinv: Tensor, pix: Tensor, W: int, d_d: Tensor, d_o: Tensor) -> Tuple[Tensor, Tensor]:
    z = torch.zeros(24, dtype=torch.float32, device=pix.device)          # (one fill for both accumulation targets)
    d_pose, d_kinv = z[:12].view(3, 4), z[12:21].view(3, 3)
    _lib.call("mcnerf_raygen_bwd", pose, kinv, pix, pix.numel(), W,
              d_d, d_o, d_pose, d_kinv, _stream())
    return d_pose, d_kinv


@dataclass
class MlpSave:
    """Workspaces written by mlp_fwd(save=True) and consumed by mlp_bwd / mlp_dw.  In the 16-bit modes `act`, `enc`
    `sh` and `mask` are byte / word buffers in the fragment-major layouts of csrc/mcnerf_16.h."""
    capacity: int
    act: Tensor
    enc: Tensor
    sh: Optional[Tensor]
    mask: Tensor


def ws_bytes_16(net: Net, capacity: int, which: int, precision: str = "f16") -> int:
    return int(_lib.lib().mcnerf_ws_bytes_16(net.depth, net.width, DTYPE16[precision], int(capacity), which))


def alloc_save(net: Net, capacity: int, device, precision: str = "f32") -> MlpSave:
    capacity = max(int(capacity), 1)
    if is16(precision):
        return MlpSave(capacity,
                       torch.empty(ws_bytes_16(net, capacity, 0, precision), dtype=torch.uint8, device=device),
                       torch.empty(ws_bytes_16(net, capacity, 1, precision), dtype=torch.uint8, device=device),
                       torch.empty(ws_bytes_16(net, capacity, 4, precision), dtype=torch.uint8, device=device),
                       torch.empty(ws_bytes_16(net, capacity, 2, precision) // 4, dtype=torch.int32, device=device))
    return MlpSave(capacity,
                   torch.empty((net.depth + 2) * capacity * net.width, dtype=torch.float32, device=device),
                   torch.empty(capacity * 64, dtype=torch.float32, device=device),
                   torch.empty(capacity * net.n_shp, dtype=torch.float32, device=device),
                   torch.empty((net.depth + 2) * capacity * (net.width // 32), dtype=torch.int32, device=device))


def mlp_fwd(net: Net, params: Tensor, packed: Tensor, rays_o: Tensor, rays_d: Tensor, zgrid: Tensor,
            jitter: Optional[Tensor], barf_w: Tensor, out: Tensor, idx: Optional[Tensor] = None,
            count: Optional[Tensor] = None, max_rows: int = 0, save: Optional[MlpSave] = None,
            precision: str = "f32", *, z_rows: Optional[Tensor] = None) -> None:
    """`z_rows` [n_rays, S]: per-ray sample depths instead of the shared grid `zgrid` [S] (the dense fine pass on sample_pdf's rows,
    jitter None: the rows hold it)."""
    n_rays = rays_d.shape[0]
    zgrid, S, zs = _depths(zgrid, z_rows, n_rays)
    assert out.numel() == n_rays * S * 4
    if is16(precision):
        _lib.call("mcnerf_mlp_fwd_16", *net.triple, DTYPE16[precision], params, packed16_split(net, packed, precision)[0], rays_o, rays_d,
                  zgrid, zs, jitter, barf_w, idx, count, int(max_rows), n_rays, S,
                  out, save.act if save else None, save.capacity if save else 0,
                  save.enc if save else None, save.mask if save else None,
                  save.sh if save else None, _stream())
        return
    _lib.call("mcnerf_mlp_fwd", *net.triple, params, packed, rays_o, rays_d, zgrid, zs,
              jitter, barf_w, idx, count, int(max_rows), n_rays, S,
              out, save.act if save else None, save.capacity if save else 0,
              save.enc if save else None, save.sh if save else None,
              save.mask if save else None, _stream())


def seed_word(device) -> Tensor:
    """The key word of a device-side draw (sample_perm, the ray-batch forwards, cap_random): one int32 [1] from torch's device
    generator, so torch.manual_seed reproduces it."""
    return torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int32, device=device)


def sample_perm(n: int, batch: int, device, seed: Optional[Tensor] = None) -> Tensor:
    """randperm(n)[:batch] (model/mc_nerf.py:329) in one kernel: `batch` distinct uniformly random ids of [0, n) in random
    order (int64); the key is a device word drawn from torch's device generator, so torch.manual_seed reproduces it."""
    if seed is None:
        seed = seed_word(device)
    out = torch.empty(batch, dtype=torch.int64, device=device)
    _lib.call("mcnerf_sample_perm", out, int(n), int(batch), seed, _stream())
    return out


def ray_segments(batch: int, K: int):
    """seg_start [K+1] of a `batch`-ray step over K cameras: segment k holds n_k = batch // K + (1 if k < batch % K else 0)
    consecutive rays (sizes differ by at most one and sum to batch)."""
    batch, K = int(batch), int(K)
    if K < 1 or batch < 0:
        raise ValueError(f"ray_segments needs K >= 1 and batch >= 0, got batch = {batch}, K = {K}")
    q, r = divmod(batch, K)
    start = [0]
    for k in range(K):
        start.append(start[-1] + q + (1 if k < r else 0))
    return start


def ray_segment_index(batch: int, K: int, device) -> Tensor:
    """The segment of every ray of `ray_segments(batch, K)` as a device int64 [batch], from arithmetic on an arange: no host ->
    device copy of a table and no host synchronisation (the first r = batch % K segments hold q + 1 rays, the others q)."""
    q, r = divmod(int(batch), int(K))
    i = torch.arange(int(batch), dtype=torch.int64, device=device)
    head = r * (q + 1)
    return torch.where(i < head, i // (q + 1), r + (i - head) // max(q, 1))


def _seg_arrays(seg_cam, seg_start):
    import ctypes
    cams, start = [int(c) for c in seg_cam], [int(s) for s in seg_start]
    if len(start) != len(cams) + 1:
        raise _lib.McnerfError(f"seg_start must hold len(seg_cam) + 1 = {len(cams) + 1} entries, got {len(start)}")
    return (ctypes.c_int32 * len(cams))(*cams), (ctypes.c_int32 * len(start))(*start), len(cams), start[-1]


def _lens_arg(lens: Tensor, C: int) -> Tensor:
    if lens.dim() != 2 or tuple(lens.shape) != (C, 2):
        raise _lib.McnerfError(f"lens must be [C = {C}, 2] (k1, k2), got {tuple(lens.shape)}")
    return lens


def _ray_batch_fwd(symbol: str, pose: Tensor, kinv: Tensor, lens: Optional[Tensor], seg_cam, seg_start, H: int, W: int,
                   images: Optional[Tensor], pix: Optional[Tensor], seed: Optional[Tensor], draw_seed: bool):
    """Both forwards: `symbol` with `lens` [C,2] behind kinv, or without it (None).  draw_seed: the key word is still to be drawn."""
    cams, start, K, n = _seg_arrays(seg_cam, seg_start)
    dev = pose.device
    lens_args = () if lens is None else (_lens_arg(lens, int(pose.shape[0])),)
    if draw_seed:
        seed = seed_word(dev)
    if pix is not None and pix.numel() != n:
        raise _lib.McnerfError(f"pix must hold seg_start[-1] = {n} ids, got {pix.numel()}")
    if images is not None and (images.dim() != 3 or images.shape[0] != pose.shape[0] or images.shape[1] != H * W):
        raise _lib.McnerfError(f"images must be [C = {pose.shape[0]}, H*W = {H * W}, channels], got {tuple(images.shape)}")
    pix_out = torch.empty(n, dtype=torch.int64, device=dev)
    d = torch.empty(n, 3, dtype=torch.float32, device=dev)
    o = torch.empty_like(d)
    gt = torch.empty_like(d) if images is not None else None
    _lib.call(symbol, pose, kinv, *lens_args, int(pose.shape[0]), cams, start, K, n, int(H), int(W),
              pix, seed, images, int(images.shape[-1]) if images is not None else 0,
              pix_out, d, o, gt, _stream())
    return pix_out, d, o, gt


def _ray_batch_bwd(symbol: str, pose: Tensor, kinv: Tensor, lens: Optional[Tensor], seg_cam, seg_start, W: int, pix: Tensor, d_d: Tensor,
                   d_o: Tensor):
    """Both backwards -> (d_pose [C,3,4], d_kinv [C,3,3]) and, with `lens`, d_lens [C,2]: views of one zero-filled buffer."""
    cams, start, K, n = _seg_arrays(seg_cam, seg_start)
    C = int(pose.shape[0])
    lens_args = () if lens is None else (_lens_arg(lens, C),)
    z = torch.zeros(C * (21 if lens is None else 23), dtype=torch.float32, device=pose.device)     # (one fill for every accumulation target)
    outs = (z[:C * 12].view(C, 3, 4), z[C * 12:C * 21].view(C, 3, 3)) + (() if lens is None else (z[C * 21:].view(C, 2),))
    if pix.numel() != n or d_d.numel() != 3 * n or d_o.numel() != 3 * n:
        raise _lib.McnerfError(f"pix / d_rays_d / d_rays_o must hold seg_start[-1] = {n} rays")
    _lib.call(symbol, pose, kinv, *lens_args, C, cams, start, K, n, int(W), pix,
              d_d, d_o, *outs, _stream())
    return outs


def ray_batch_fwd(pose: Tensor, kinv: Tensor, seg_cam, seg_start, H: int, W: int, images: Optional[Tensor] = None,
                  pix: Optional[Tensor] = None, seed: Optional[Tensor] = None):
    """The ray preamble of a multi-camera step in one launch.  pose [C,3,4], kinv [C,3,3]; segment k = rays
    [seg_start[k], seg_start[k+1]) of camera seg_cam[k] (host lists; they travel as kernel arguments).  `pix` [n] int64 injects the
    pixels; otherwise segment k draws the permutation of `sample_perm` keyed by seed + k * 0x9E3779B9 (`seed`: a device int32 word,
    drawn from torch's device generator when not given, as `sample_perm` does).  `images` [C, H*W, 3|4] uint8 on the device gives the
    ground truth.  -> (pix [n] int64, rays_d [n,3], rays_o [n,3], gt [n,3] | None)"""
    return _ray_batch_fwd("mcnerf_ray_batch_fwd", pose, kinv, None, seg_cam, seg_start, H, W, images, pix, seed,
                          draw_seed=pix is None and seed is None and pose.is_cuda)


def ray_batch_bwd(pose: Tensor, kinv: Tensor, seg_cam, seg_start, W: int, pix: Tensor, d_d: Tensor, d_o: Tensor) -> Tuple[Tensor, Tensor]:
    """Backward of `ray_batch_fwd`: -> (d_pose [C,3,4], d_kinv [C,3,3]); rows of cameras not in the table are exactly zero."""
    return _ray_batch_bwd("mcnerf_ray_batch_bwd", pose, kinv, None, seg_cam, seg_start, W, pix, d_d, d_o)


def lens_ray_batch_fwd(pose: Tensor, kinv: Tensor, lens: Tensor, seg_cam, seg_start, H: int, W: int, images: Optional[Tensor] = None,
                       pix: Optional[Tensor] = None, seed: Optional[Tensor] = None):
    """`ray_batch_fwd` with per-camera radial lens distortion (`lens_model` = "radial"): lens [C,2] = (k1, k2); every
    ray's lifted pixel is undistorted by eight safeguarded Newton steps before the rotation (csrc/mcnerf_lens.h).  Pixels (the same
    draw from the same seed word) and ground truth as `ray_batch_fwd`; at lens = 0 every output has its bits.  CUDA/HIP tensors only.
    -> (pix [n] int64, rays_d [n,3], rays_o [n,3], gt [n,3] | None)"""
    return _ray_batch_fwd("mcnerf_lens_ray_batch_fwd", pose, kinv, lens, seg_cam, seg_start, H, W, images, pix, seed,
                          draw_seed=pix is None and seed is None)


def lens_ray_batch_bwd(pose: Tensor, kinv: Tensor, lens: Tensor, seg_cam, seg_start, W: int, pix: Tensor, d_d: Tensor,
                       d_o: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """Backward of `lens_ray_batch_fwd`: -> (d_pose [C,3,4], d_kinv [C,3,3], d_lens [C,2]); rows of cameras not in the table are
    exactly zero, a camera listed twice receives the sum."""
    return _ray_batch_bwd("mcnerf_lens_ray_batch_bwd", pose, kinv, lens, seg_cam, seg_start, W, pix, d_d, d_o)


def upload_f32(host_vals: Tensor, device) -> Tensor:
    """A small fp32 host tensor (<= 16 values) as a fresh device tensor, stream-ordered and without a host-device copy
    (the values travel as kernel arguments): the host never waits for the kernels already queued."""
    hv = host_vals.detach().reshape(-1).float().contiguous()
    assert hv.device.type == "cpu" and hv.numel() <= 16
    out = torch.empty(hv.numel(), dtype=torch.float32, device=device)
    _lib.call("mcnerf_upload_f32", out, hv.data_ptr(), hv.numel(), _stream())
    return out


def encode(x: Tensor, barf_w: Tensor) -> Tensor:
    """SinCosEmbedding.forward (model/net_block.py:20-35): [n,3] -> [n, 3 + 6 F] with F = len(barf_w) frequencies (10: 63)."""
    n, F = x.shape[0], barf_w.numel()
    out = torch.empty(n, 3 + 6 * F, dtype=torch.float32, device=x.device)
    _lib.call("mcnerf_encode", x, barf_w, n, F, out, _stream())
    return out


def mlp_apply(net: Net, params: Tensor, packed: Tensor, x_enc: Tensor, dirs: Tensor) -> Tensor:
    """CorseFine_NeRF.forward (model/net_block.py:67-78) on given encodings: [n,63], [n,3] -> [n,4] (exact-fp32 kernel)."""
    n = x_enc.shape[0]
    out = torch.empty(n, 4, dtype=torch.float32, device=x_enc.device)
    _lib.call("mcnerf_mlp_apply", *net.triple, params, packed, x_enc, dirs, n, out, _stream())
    return out


def sync_finish(arena: Tensor, n_grad: int, world: int, local_flags: Tensor, asym: Tensor) -> None:
    """arena[:n_grad] /= world; asym += any(arena[n_grad:] != world * local_flags) -- the finish of FlatGradSync's one all-reduce
    in one launch."""
    _lib.call("mcnerf_sync_finish", arena, int(n_grad), int(arena.numel() - n_grad), int(world), local_flags,
              asym, _stream())


def encode_bwd(x: Tensor, barf_w: Tensor, d_out: Tensor) -> Tensor:
    """Backward of `encode`: d_out [n, 3 + 6 F] -> d_x [n,3]."""
    n = x.shape[0]
    d_x = torch.empty(n, 3, dtype=torch.float32, device=x.device)
    _lib.call("mcnerf_encode_bwd", x, barf_w, n, barf_w.numel(), d_out, d_x, _stream())
    return d_x


def mlp_apply_save(net: Net, params: Tensor, packed: Tensor, x_enc: Tensor, dirs: Tensor) -> Tuple[Tensor, MlpSave]:
    """`mlp_apply` that keeps the operands of its backward (exact-fp32 workspaces)."""
    n = x_enc.shape[0]
    out = torch.empty(n, 4, dtype=torch.float32, device=x_enc.device)
    save = alloc_save(net, n, x_enc.device, "f32")
    _lib.call("mcnerf_mlp_apply_save", *net.triple, params, packed, x_enc, dirs, n, out,
              save.act, save.capacity, save.enc, save.sh, save.mask, _stream())
    return out, save


def mlp_apply_bwd(net: Net, params: Tensor, packed: Tensor, dirs: Tensor, out: Tensor, d_out: Tensor, save: MlpSave,
                  grads: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """Backward of `mlp_apply_save`: -> (d_x_enc [n,63], d_dirs [n,3]); the parameter gradients are ACCUMULATED into the flat
    `grads` (layout of the parameter buffer) unless it is None."""
    n = dirs.shape[0]
    dev = dirs.device
    dy, dsh = torch.empty_like(save.act), torch.empty_like(save.sh)
    d_x = torch.empty(n, net.n_enc, dtype=torch.float32, device=dev)
    z = torch.zeros(n * 3 + 1, dtype=torch.float32, device=dev)          # (d_dirs accumulator + the zero sample depth, one fill)
    d_dirs = z[:n * 3].view(n, 3)
    _lib.call("mcnerf_mlp_apply_bwd", *net.triple, params, packed, dirs, z[n * 3:], n, out, d_out,
              save.mask, save.capacity, save.enc, save.sh, dy, dsh, d_x, d_dirs, _stream())
    if grads is not None:
        mlp_dw(net, save, dy, dsh, grads, n)
    return d_x, d_dirs


def mlp_bwd(net: Net, params: Tensor, packed: Tensor, rays_o: Tensor, rays_d: Tensor, zgrid: Tensor,
            jitter: Optional[Tensor], barf_w: Tensor, out: Tensor, d_out: Tensor, save: MlpSave,
            dy: Tensor, dsh: Tensor, d_rays_o: Optional[Tensor], d_rays_d: Optional[Tensor],
            idx: Optional[Tensor] = None, count: Optional[Tensor] = None, max_rows: int = 0,
            precision: str = "f32", gmax: Optional[Tensor] = None, *, z_rows: Optional[Tensor] = None) -> None:
    """`z_rows`: as mlp_fwd's (the depths the forward was run on)."""
    n_rays = rays_d.shape[0]
    zgrid, S, zs = _depths(zgrid, z_rows, n_rays)
    if is16(precision):
        _lib.call("mcnerf_mlp_bwd_16", *net.triple, DTYPE16[precision], params, packed16_split(net, packed, precision)[1], rays_o, rays_d,
                  zgrid, zs, jitter, barf_w, idx, count, int(max_rows), n_rays, S,
                  out, d_out, save.mask, save.capacity, save.enc, save.sh,
                  dy, dsh, d_rays_o, d_rays_d, gmax, _stream())
        return
    args = [*net.triple, params, packed, rays_o, rays_d, zgrid, zs,
            jitter, barf_w, idx, count, int(max_rows), n_rays, S,
            out, d_out, save.mask, save.capacity, save.enc, save.sh,
            dy, dsh, d_rays_o, d_rays_d]
    _lib.call("mcnerf_mlp_bwd", *args, _stream())


def mlp_dw(net: Net, save: MlpSave, dy: Tensor, dsh: Tensor, grads: Tensor, rows: int,
           count: Optional[Tensor] = None, precision: str = "f32", gmax: Optional[Tensor] = None) -> None:
    if is16(precision):
        _lib.call("mcnerf_mlp_dw_16", *net.triple, DTYPE16[precision], count, int(rows), save.act,
                  save.enc, dy, dsh, save.capacity, grads,
                  gmax, _stream())
        return
    args = [*net.triple, count, int(rows), save.act, save.enc, dy, dsh, save.capacity, grads]
    _lib.call("mcnerf_mlp_dw", *args, _stream())


def composite_fwd(sig_rgb: Tensor, rays_d: Tensor, zgrid: Tensor, jitter: Optional[Tensor], eps: Tensor,
                  eps_sel: Optional[Tensor] = None, white_back: bool = True, want_depth: bool = False, *,
                  z_rows: Optional[Tensor] = None):
    """-> rgb [N,3], depth [N,1] | None, opacity [N,1] | None, w_sel [N,S] | None, wmax_bits | None.
    `z_rows` [N,S]: per-ray depths instead of the shared grid (S is then its last dimension)."""
    N = rays_d.shape[0]
    zgrid, S, zs = _depths(zgrid, z_rows, N)
    dev = rays_d.device
    rgb = torch.empty(N, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(N, 1, dtype=torch.float32, device=dev) if want_depth else None
    opac = torch.empty(N, 1, dtype=torch.float32, device=dev) if want_depth else None
    w_sel = torch.empty(N, S, dtype=torch.float32, device=dev) if eps_sel is not None else None
    wmax = torch.zeros(1, dtype=torch.int32, device=dev) if eps_sel is not None else None
    _lib.call("mcnerf_composite_fwd", sig_rgb, rays_d, zgrid, zs, jitter, eps, eps_sel, N, S,
              int(bool(white_back)), rgb, depth, opac, w_sel, wmax, _stream())
    return rgb, depth, opac, w_sel, wmax


def _bwd_out(d_rgb: Tensor, S: int, want_gmax: bool):
    """-> (d_sig_rgb [N,S,4], the zeroed word of max|d_sig_rgb| or None, what a composite backward returns: (d, gmax) with want_gmax, else d)"""
    d = torch.empty(d_rgb.shape[0], S, 4, dtype=torch.float32, device=d_rgb.device)
    gmax = torch.zeros(1, dtype=torch.int32, device=d_rgb.device) if want_gmax else None
    return d, gmax, ((d, gmax) if want_gmax else d)


def _moments_of(d_dist: Optional[Tensor], moments: Optional[Tensor], N: int) -> Optional[Tensor]:
    """The `moments` argument of a composite backward: those of `distortion_fwd`, checked, with d_dist; None without it."""
    if d_dist is None:
        return None
    if moments is None or tuple(moments.shape) != (N, DIST_MOMENT_BYTES):
        raise _lib.McnerfError(f"d_dist needs the moments [{N}, {DIST_MOMENT_BYTES}] of distortion_fwd, got "
                               + ("None" if moments is None else str(tuple(moments.shape))))
    return moments


def _gather_out(src: Tensor, dims: int, layout: str, seg_cam, seg_start, pix: Tensor):
    """-> (cams, start, K, n, out [n]) of a gather over the per-camera pixels `src` (`dims` dimensions; `layout` words the refusal)."""
    cams, start, K, n = _seg_arrays(seg_cam, seg_start)
    if src.dim() != dims or pix.numel() != n:
        raise _lib.McnerfError(f"{layout} and pix must hold seg_start[-1] = {n} ids, got {tuple(src.shape)}, {pix.numel()}")
    return cams, start, K, n, torch.empty(n, dtype=torch.float32, device=pix.device)


def composite_bwd(sig_rgb: Tensor, zgrid: Tensor, jitter: Optional[Tensor], eps: Tensor, d_rgb: Tensor,
                  white_back: bool = True, want_gmax: bool = False, *, z_rows: Optional[Tensor] = None):
    """-> d_sig_rgb [N,S,4] (and, with want_gmax, the int32 word holding max|d_sig_rgb| as float bits); `z_rows` as composite_fwd's"""
    N = d_rgb.shape[0]
    zgrid, S, zs = _depths(zgrid, z_rows, N)
    d, gmax, out = _bwd_out(d_rgb, S, want_gmax)
    _lib.call("mcnerf_composite_bwd", sig_rgb, zgrid, zs, jitter, eps, d_rgb, N, S,
              int(bool(white_back)), d, gmax, _stream())
    return out


# --------------------------------------------------------------------------- alpha-mask supervision (the extension library)
def front_weight(sig_rgb: Tensor, zgrid: Tensor, jitter: Optional[Tensor], eps: Tensor, *, z_rows: Optional[Tensor] = None) -> Tensor:
    """-> fg [N] = sum_{j < S-1} w_j of the rgb composite's weights of `composite_fwd` on the same inputs: every weight but the
    far-plane sample's (delta = 1e10), which takes whatever transmittance is left."""
    N = sig_rgb.shape[0]
    zgrid, S, zs = _depths(zgrid, z_rows, N)
    fg = torch.empty(N, dtype=torch.float32, device=sig_rgb.device)
    _ext.call("mcnerf_ext_front_weight", sig_rgb, zgrid, zs, jitter, eps, N, S, fg, _stream())
    return fg


def composite_bwd_front(sig_rgb: Tensor, zgrid: Tensor, jitter: Optional[Tensor], eps: Tensor, d_rgb: Tensor, d_fg: Optional[Tensor],
                        white_back: bool = True, want_gmax: bool = False, *, z_rows: Optional[Tensor] = None):
    """`composite_bwd` of  sum rgb * d_rgb + sum fg * d_fg  (d_fg [N]); with d_fg None the bits of `composite_bwd`."""
    N = d_rgb.shape[0]
    zgrid, S, zs = _depths(zgrid, z_rows, N)
    d, gmax, out = _bwd_out(d_rgb, S, want_gmax)
    _ext.call("mcnerf_ext_composite_bwd_front", sig_rgb, zgrid, zs, jitter, eps, d_rgb, d_fg, N, S,
              int(bool(white_back)), d, gmax, _stream())
    return out


def gather_alpha(images_u8: Tensor, seg_cam, seg_start, pix: Tensor) -> Tensor:
    """images_u8 [C, H*W, 3|4] uint8 on the device, pix [n] int64 (segment k = rays [seg_start[k], seg_start[k+1]) of camera
    seg_cam[k]; host lists) -> alpha [n] fp32 = a / 255 of the drawn pixels, ones for 3-channel images."""
    cams, start, K, n, alpha = _gather_out(images_u8, 3, "images must be [C, H*W, channels]", seg_cam, seg_start, pix)
    _ext.call("mcnerf_ext_gather_alpha", images_u8, int(images_u8.shape[0]), int(images_u8.shape[1]), int(images_u8.shape[2]),
              cams, start, K, pix, n, alpha, _stream())
    return alpha


def mask_loss(fg_c: Tensor, fg_f: Optional[Tensor], alpha: Tensor, weight: float):
    """-> out [2] = (weight * m, m), m = mean (fg_c - alpha)^2 + mean (fg_f - alpha)^2, and d_fg_c, d_fg_f | None =
    (2 weight / n) (fg - alpha); one launch, deterministic."""
    n = fg_c.numel()
    if alpha.numel() != n or (fg_f is not None and fg_f.numel() != n):
        raise _lib.McnerfError(f"fg_c, fg_f and alpha must hold the same {n} rays")
    out = torch.zeros(MASK_LOSS_OUT, dtype=torch.float32, device=fg_c.device)      # [3] = the kernel's arrival counter: zero on entry
    d_c = torch.empty_like(fg_c)
    d_f = torch.empty_like(fg_f) if fg_f is not None else None
    _ext.call("mcnerf_ext_mask_loss", fg_c, fg_f, alpha, n, float(weight), out, d_c, d_f, _stream())
    return out[:2], d_c, d_f


# --------------------------------------------------------------------------- distortion loss (the regulariser library)
def _z_span(near: float, far: float):
    """(z_near, z_scale = 1 / (far - near)) of s = (z - near) z_scale; an empty range gives the infinity the library refuses."""
    near, far = float(near), float(far)
    return near, (1.0 / (far - near) if far != near else float("inf"))


def distortion_fwd(sig_rgb: Tensor, zgrid: Tensor, jitter: Optional[Tensor], eps: Tensor, near: float, far: float, *,
                   z_rows: Optional[Tensor] = None):
    """-> (dist [N], moments [N, 16] uint8) of the rgb composite's weights w of `composite_fwd` on the same inputs:
    dist = sum_ij w_i w_j |s_i - s_j| + (1/3) sum_{j<S-1} w_j^2 (s_{j+1} - s_j), s = (z - near) / (far - near); the far-plane sample
    takes part in the pair term and has no interval term.  The depth rows must be non-decreasing.  `moments` is opaque: the ray's
    (sum w, sum w s) in fp64, for `composite_bwd_w`."""
    N = sig_rgb.shape[0]
    zgrid, S, zs = _depths(zgrid, z_rows, N)
    dist = torch.empty(N, dtype=torch.float32, device=sig_rgb.device)
    moments = torch.empty(N, DIST_MOMENT_BYTES, dtype=torch.uint8, device=sig_rgb.device)
    _reg.call("mcnerf_reg_distortion_fwd", sig_rgb, zgrid, zs, jitter, eps, N, S, *_z_span(near, far), dist, moments, _stream())
    return dist, moments


def composite_bwd_w(sig_rgb: Tensor, zgrid: Tensor, jitter: Optional[Tensor], eps: Tensor, d_rgb: Tensor, d_fg: Optional[Tensor],
                    d_dist: Optional[Tensor], moments: Optional[Tensor], near: float, far: float, white_back: bool = True,
                    want_gmax: bool = False, *, z_rows: Optional[Tensor] = None):
    """`composite_bwd` of  sum rgb * d_rgb + sum fg * d_fg + sum dist * d_dist  (d_fg, d_dist [N] or None; d_dist with the `moments`
    of `distortion_fwd` on the same inputs, near and far).  With d_dist None the bits of `composite_bwd_front`, with both None those
    of `composite_bwd`."""
    N = d_rgb.shape[0]
    zgrid, S, zs = _depths(zgrid, z_rows, N)
    moments = _moments_of(d_dist, moments, N)
    d, gmax, out = _bwd_out(d_rgb, S, want_gmax)
    _reg.call("mcnerf_reg_composite_bwd_w", sig_rgb, zgrid, zs, jitter, eps, d_rgb, d_fg, d_dist, moments,
              *_z_span(near, far), N, S, int(bool(white_back)), d, gmax, _stream())
    return out


# --------------------------------------------------------------------------- depth supervision (the geometry library)
def expected_depth(sig_rgb: Tensor, zgrid: Tensor, jitter: Optional[Tensor], eps: Tensor, *, z_rows: Optional[Tensor] = None) -> Tensor:
    """-> zexp [N] = sum_j w_j z_j of the rgb composite's weights of `composite_fwd` on the same inputs, z_j = fl32(z + jitter): the
    far-plane sample (delta = 1e10) takes part at its depth.  Not `composite_fwd`'s `depth` (noise-free, |d|-scaled weights)."""
    N = sig_rgb.shape[0]
    zgrid, S, zs = _depths(zgrid, z_rows, N)
    zexp = torch.empty(N, dtype=torch.float32, device=sig_rgb.device)
    _geo.call("mcnerf_geo_depth_fwd", sig_rgb, zgrid, zs, jitter, eps, N, S, zexp, _stream())
    return zexp


def composite_bwd_z(sig_rgb: Tensor, zgrid: Tensor, jitter: Optional[Tensor], eps: Tensor, d_rgb: Tensor, d_fg: Optional[Tensor],
                    d_dist: Optional[Tensor], moments: Optional[Tensor], d_zexp: Optional[Tensor], near: float, far: float,
                    white_back: bool = True, want_gmax: bool = False, *, z_rows: Optional[Tensor] = None):
    """`composite_bwd` of  sum rgb * d_rgb + sum fg * d_fg + sum dist * d_dist + sum zexp * d_zexp  (d_fg, d_dist, d_zexp [N] or None;
    d_dist with the `moments` of `distortion_fwd` on the same inputs, near and far).  With d_zexp None the bits of `composite_bwd_w`."""
    N = d_rgb.shape[0]
    zgrid, S, zs = _depths(zgrid, z_rows, N)
    moments = _moments_of(d_dist, moments, N)
    if d_zexp is not None and d_zexp.numel() != N:
        raise _lib.McnerfError(f"d_zexp must hold the {N} rays of d_rgb, got {tuple(d_zexp.shape)}")
    d, gmax, out = _bwd_out(d_rgb, S, want_gmax)
    _geo.call("mcnerf_geo_composite_bwd_z", sig_rgb, zgrid, zs, jitter, eps, d_rgb, d_fg, d_dist, moments,
              d_zexp, *_z_span(near, far), N, S, int(bool(white_back)), d, gmax, _stream())
    return out


def gather_depth(depth: Tensor, seg_cam, seg_start, pix: Tensor) -> Tensor:
    """depth [C, H*W] fp32 on the device (ray distance in world units), pix [n] int64 (segment k = rays [seg_start[k], seg_start[k+1])
    of camera seg_cam[k]; host lists) -> d_gt [n] fp32: the stored value where it is finite and > 0, else 0.0 (no measurement; a pixel
    id outside the image as well)."""
    cams, start, K, n, out = _gather_out(depth, 2, "depth must be [C, H*W]", seg_cam, seg_start, pix)
    _geo.call("mcnerf_geo_gather_depth", depth, int(depth.shape[0]), int(depth.shape[1]), cams, start, K, pix, n, out, _stream())
    return out


def depth_loss(zexp_c: Tensor, zexp_f: Optional[Tensor], d_gt: Tensor, near: float, far: float, weight: float):
    """-> out [3] = (weight * m, m, n_valid), m = (1 / max(n_valid, 1)) sum_valid (s(zexp_c) - s(d_gt))^2 + (s(zexp_f) - s(d_gt))^2 with
    s(z) = (z - near) / (far - near) over the rays whose target is finite and > 0, and d_c, d_f | None =
    (2 weight z_scale / n_valid) (s(zexp) - s(d_gt)) on those rays, exactly 0 on the others; two launches, deterministic."""
    n = zexp_c.numel()
    if d_gt.numel() != n or (zexp_f is not None and zexp_f.numel() != n):
        raise _lib.McnerfError(f"zexp_c, zexp_f and d_gt must hold the same {n} rays")
    out = torch.zeros(DEPTH_LOSS_OUT, dtype=torch.float32, device=zexp_c.device)   # [3] = the kernel's arrival counter: zero on entry
    d_c = torch.empty_like(zexp_c)
    d_f = torch.empty_like(zexp_f) if zexp_f is not None else None
    _geo.call("mcnerf_geo_depth_loss", zexp_c, zexp_f, d_gt, n, *_z_span(near, far), float(weight), out, d_c, d_f, _stream())
    return out[:3], d_c, d_f


def _list_buffers(N: int, S: int, prefill: bool, idx: Optional[Tensor], dev):
    """What an ordered (ray, sample) list over [N, S] needs (csrc/mcnerf_compact.h): idx [N*S,2] (or the caller's), count [1], the two
    [N] workspaces and, with `prefill`, the [N,S,4] output the count kernel fills with the defaults."""
    if idx is None:
        idx = torch.empty(N * S, 2, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    rc = torch.empty(N, dtype=torch.int32, device=dev)
    ro = torch.empty(N, dtype=torch.int32, device=dev)
    return idx, count, rc, ro, torch.empty(N, S, 4, dtype=torch.float32, device=dev) if prefill else None


def _hit_flags(name: str, hit: Tensor, N: int) -> Tensor:
    if hit.dim() != 1 or hit.shape[0] != N:
        raise _lib.McnerfError(f"{name}: hit must be [N = {N}] int32, got {tuple(hit.shape)}")
    return hit


def select_fine(w_sel: Tensor, wmax: Tensor, thresh: float, scale: int, sigma_default: float,
                prefill: bool = True, hit: Optional[Tensor] = None):
    """-> idx [N*Sc*scale,2] int32 (first *count rows valid), count [1] int32, out_f [N,Sf,4] | None
    `hit` [N] int32: only rays with hit[n] != 0 are listed; the hit library's entry point (include/mcnerf_hit.h)."""
    N, Sc = w_sel.shape
    idx, count, rc, ro, out_f = _list_buffers(N, Sc * scale, prefill, None, w_sel.device)
    if hit is not None:
        _hit.call("mcnerf_hit_select_fine", w_sel, wmax, float(thresh), N, Sc, scale, float(sigma_default), rc, ro, idx, count, out_f,
                  _hit_flags("select_fine", hit, N), _stream())
    else:
        _lib.call("mcnerf_select_fine", w_sel, wmax, float(thresh), N, Sc, scale,
                  float(sigma_default), rc, ro, idx,
                  count, out_f, _stream())
    return idx, count, out_f


def list_rays(hit: Tensor, S: int, sigma_default: float, prefill: bool = True, idx: Optional[Tensor] = None):
    """-> idx [N*S,2] int32 (first *count rows valid, torch.nonzero order), count [1] int32 = S * (rays with hit[n] != 0), out [N,S,4] |
    None: every (ray, sample) pair of the rays that hit the scene box and the (sigma_default, 1, 1, 1) prefill of all rays
    (include/mcnerf_hit.h: mcnerf_hit_list_rays).  No host synchronisation.  `idx`: the caller's own list buffer (rows beyond *count are
    left as they are)."""
    N, S = hit.shape[0], int(S)
    _hit_flags("list_rays", hit, N)
    if idx is not None and idx.numel() < N * S * 2:
        raise _lib.McnerfError(f"list_rays: idx must hold N * S = {N * S} pairs, got {tuple(idx.shape)}")
    idx, count, rc, ro, out = _list_buffers(N, S, prefill, idx, hit.device)
    _hit.call("mcnerf_hit_list_rays", hit, N, S, float(sigma_default), rc, ro, idx, count, out, _stream())
    return idx, count, out


def sample_pdf(w_sel: Tensor, zgrid: Optional[Tensor], jitter: Optional[Tensor], u: Tensor, out: Optional[Tensor] = None, *,
               z_rows: Optional[Tensor] = None) -> Tensor:
    """Inverse-CDF hierarchical sampling (include/mcnerf.h: mcnerf_sample_pdf): coarse selection weights w_sel [N,Sc], the coarse
    grid zgrid [Sc], jitter [N] | None and uniform draws u [N,I] -> z_all [N,Sc+I] = sort(coarse depths ++ importance samples).
    Not differentiable (z_all is a constant of the fine pass, as in vanilla NeRF).
    `out`: the caller's own z_all (fp32, contiguous, [N,Sc+I], on w_sel's device), e.g. rows of a larger buffer; it is returned.
    `z_rows` [N,Sc]: the coarse depths of every ray (zgrid and jitter None); the bounds library's entry point
    (include/mcnerf_box.h: mcnerf_box_sample_pdf_rows), the same device code."""
    N, Sc = w_sel.shape
    if z_rows is not None:
        if zgrid is not None or jitter is not None or tuple(z_rows.shape) != (N, Sc):
            raise _lib.McnerfError(f"sample_pdf: z_rows must be [N = {N}, Sc = {Sc}] with zgrid and jitter None, got {tuple(z_rows.shape)}")
    elif zgrid.numel() != Sc or (jitter is not None and jitter.numel() != N):
        raise _lib.McnerfError(f"sample_pdf: w_sel [N,Sc] {tuple(w_sel.shape)}, zgrid [Sc] {tuple(zgrid.shape)}, u [N,I] {tuple(u.shape)}")
    if u.dim() != 2 or u.shape[0] != N:
        raise _lib.McnerfError(f"sample_pdf: w_sel [N,Sc] {tuple(w_sel.shape)}, u [N,I] {tuple(u.shape)}")
    I = u.shape[1]
    if out is None:
        out = torch.empty(N, Sc + I, dtype=torch.float32, device=w_sel.device)
    elif tuple(out.shape) != (N, Sc + I) or out.dtype != torch.float32 or out.device != w_sel.device or not out.is_contiguous():
        raise _lib.McnerfError(f"sample_pdf: out must be a contiguous fp32 [N = {N}, Sc + I = {Sc + I}] tensor on {w_sel.device}, got "
                               f"{out.dtype} {tuple(out.shape)} on {out.device}{'' if out.is_contiguous() else ', not contiguous'}")
    if z_rows is not None:
        _box.call("mcnerf_box_sample_pdf_rows", w_sel, z_rows, u, N, Sc, I, out, _stream())
    else:
        _lib.call("mcnerf_sample_pdf", w_sel, zgrid, jitter, u, N, Sc, I, out, _stream())
    return out


# --------------------------------------------------------------------------- per-ray sample bounds (include/mcnerf_box.h)
def ray_depths(rays_o: Tensor, rays_d: Tensor, box, near: float, far: float, jitter: Optional[Tensor], zgrid_c: Tensor,
               zgrid_f: Optional[Tensor] = None, want_span: bool = True, want_hit: bool = False):
    """Per-ray depth rows from the scene box (mcnerf_box_ray_depths; the rule: include/mcnerf_box.h): rays [N,3], box = (xmin, ymin,
    zmin, xmax, ymax, zmax), jitter [N] | None, the grids zgrid_c [Sc] and zgrid_f [Sf] | None -> z_c [N,Sc], z_f [N,Sf] | None,
    span [N,2] = (lo, hi) | None.  One launch, no host synchronisation; constants of the backward.
    `want_hit`: a fourth result, hit [N] int32 = 1 iff the box clips the ray, from the same launch of the same kernel in the hit library
    (include/mcnerf_hit.h: mcnerf_hit_ray_depths); the other three are the same bits.
    `box` a Tensor [6] fp32 on the device (ops.voxel_box's): the fit library's entry point (include/mcnerf_fit.h: mcnerf_fit_ray_depths)
    reads the six values on the device -- the same bits again, and no value of the box reaches the host."""
    N, dev = rays_d.shape[0], rays_d.device
    on_device = isinstance(box, Tensor)
    box = box if on_device else [float(v) for v in box]
    if (box.numel() if on_device else len(box)) != 6 or tuple(rays_o.shape) != (N, 3) or tuple(rays_d.shape) != (N, 3) or (jitter is not None and jitter.numel() != N):
        raise _lib.McnerfError(f"ray_depths: rays_o / rays_d [N,3] {tuple(rays_o.shape)} / {tuple(rays_d.shape)}, a box of six numbers, jitter [N]")
    Sc, Sf = zgrid_c.numel(), 0 if zgrid_f is None else zgrid_f.numel()
    z_c = torch.empty(N, Sc, dtype=torch.float32, device=dev)
    z_f = torch.empty(N, Sf, dtype=torch.float32, device=dev) if Sf else None
    span = torch.empty(N, 2, dtype=torch.float32, device=dev) if want_span else None
    if on_device:
        hit = torch.empty(N, dtype=torch.int32, device=dev) if want_hit else None
        _fit.call("mcnerf_fit_ray_depths", rays_o, rays_d, N, box, float(near), float(far), jitter, zgrid_c, Sc, zgrid_f if Sf else None, Sf,
                  z_c, z_f, span, hit, _stream())
        return (z_c, z_f, span, hit) if want_hit else (z_c, z_f, span)
    if want_hit:
        hit = torch.empty(N, dtype=torch.int32, device=dev)
        _hit.call("mcnerf_hit_ray_depths", rays_o, rays_d, N, *box, float(near), float(far), jitter, zgrid_c, Sc, zgrid_f if Sf else None, Sf,
                  z_c, z_f, span, hit, _stream())
        return z_c, z_f, span, hit
    _box.call("mcnerf_box_ray_depths", rays_o, rays_d, N, *box, float(near), float(far), jitter, zgrid_c, Sc, zgrid_f if Sf else None, Sf,
              z_c, z_f, span, _stream())
    return z_c, z_f, span


# --------------------------------------------------------------------------- voxel sigma cache (include/mcnerf.h: mcnerf_voxel_*)
def _f32(x) -> Tensor:
    return torch.tensor(float(x), dtype=torch.float32)


def voxel_scale(G: int, bmin: float, bmax: float) -> float:
    """Cells per unit length, s = float32(G) / float32(bmax - bmin): one fp32 division on the host."""
    return float(_f32(G) / _f32(float(bmax) - float(bmin)))


def voxel_cell_edge(G: int, bmin: float, bmax: float) -> float:
    """The edge of a cell, h = float32(bmax - bmin) / float32(G): one fp32 division on the host (the fit's rule: include/mcnerf_fit.h)."""
    return float(_f32(float(bmax) - float(bmin)) / _f32(G))


def voxel_blend(beta: float) -> Tuple[float, float]:
    """(beta, 1 - beta) as the fp32 values the update kernels take (1 - beta is formed here, in fp32)."""
    b = _f32(beta)
    return float(b), float(_f32(1.0) - b)


class VoxelGrid:
    """The two device buffers of the cache and the grid's geometry: vox [G,G,G] fp32 (running raw sigma, filled with `sigma_init`),
    scratch [G,G,G] int32 (the update kernels' uint32 words, all zero between calls), over the cube [bmin, bmax]^3."""

    def __init__(self, G: int, bmin: float, bmax: float, sigma_init: float, device):
        self.G, self.bmin, self.bmax = int(G), float(_f32(bmin)), float(bmax)
        self.s = voxel_scale(G, bmin, bmax)
        self.h = voxel_cell_edge(G, bmin, bmax)
        self.vox = torch.full((self.G,) * 3, float(sigma_init), dtype=torch.float32, device=device)
        self.scratch = torch.zeros((self.G,) * 3, dtype=torch.int32, device=device)

    @property
    def geom(self):
        return self.G, self.bmin, self.s


def _voxel_rows(name: str, zgrid, jitter, z_rows: Tensor, N: int):
    if zgrid is not None or jitter is not None or z_rows.dim() != 2 or z_rows.shape[0] != N:
        raise _lib.McnerfError(f"{name}: z_rows must be [N = {N}, Sc] with zgrid and jitter None, got {tuple(z_rows.shape)}")
    return z_rows.shape[1]


def voxel_select(grid: VoxelGrid, thresh: float, rays_o: Tensor, rays_d: Tensor, zgrid: Optional[Tensor], jitter: Optional[Tensor],
                 sigma_default: float, prefill: bool = True, idx: Optional[Tensor] = None, *, z_rows: Optional[Tensor] = None,
                 hit: Optional[Tensor] = None):
    """-> idx [N*Sc,2] int32 (first *count rows valid, torch.nonzero order), count [1] int32, out_c [N,Sc,4] | None: the (ray, sample)
    pairs whose cell holds a sigma > thresh, and the (sigma_default, 1, 1, 1) prefill of the coarse pass.  No host synchronisation.
    `idx`: the caller's own list buffer (rows beyond *count are left as they are).
    `z_rows` [N,Sc]: the depths of every ray (zgrid and jitter None); the bounds library's entry point (include/mcnerf_box.h).
    `hit` [N] int32 (with `z_rows` only): only rays with hit[n] != 0 are listed; the hit library's entry point (include/mcnerf_hit.h)."""
    N = rays_d.shape[0]
    if hit is not None and z_rows is None:
        raise _lib.McnerfError("voxel_select: hit is taken together with z_rows only")
    Sc = zgrid.numel() if z_rows is None else _voxel_rows("voxel_select", zgrid, jitter, z_rows, N)
    if idx is not None and idx.numel() < N * Sc * 2:
        raise _lib.McnerfError(f"voxel_select: idx must hold N * Sc = {N * Sc} pairs, got {tuple(idx.shape)}")
    idx, count, rc, ro, out_c = _list_buffers(N, Sc, prefill, idx, rays_d.device)
    if hit is not None:
        _hit.call("mcnerf_hit_voxel_select_rows", grid.vox, *grid.geom, float(thresh), rays_o, rays_d, z_rows, N, Sc,
                  float(sigma_default), rc, ro, idx, count, out_c, _hit_flags("voxel_select", hit, N), _stream())
    elif z_rows is not None:
        _box.call("mcnerf_box_voxel_select_rows", grid.vox, *grid.geom, float(thresh), rays_o, rays_d, z_rows, N, Sc,
                  float(sigma_default), rc, ro, idx, count, out_c, _stream())
    else:
        _lib.call("mcnerf_voxel_select", grid.vox, *grid.geom, float(thresh), rays_o, rays_d, zgrid, jitter, N, Sc,
                  float(sigma_default), rc, ro, idx, count, out_c, _stream())
    return idx, count, out_c


def voxel_update(grid: VoxelGrid, beta: float, rays_o: Tensor, rays_d: Tensor, zgrid: Optional[Tensor], jitter: Optional[Tensor], sig_rgb: Tensor,
                 idx: Optional[Tensor] = None, count: Optional[Tensor] = None, max_rows: int = 0, *, z_rows: Optional[Tensor] = None) -> None:
    """The update rule on the listed (ray, sample) pairs (idx None: all N * Sc) with sigma = sig_rgb[n, j, 0]: per touched cell
    V <- (1 - beta) V + beta max(sigma), deterministic in the order of arrival; grid.scratch is all zero again afterwards.
    `z_rows` [N,Sc]: the depths of every ray (zgrid and jitter None); the bounds library's entry point (include/mcnerf_box.h)."""
    N = rays_d.shape[0]
    Sc = zgrid.numel() if z_rows is None else _voxel_rows("voxel_update", zgrid, jitter, z_rows, N)
    if sig_rgb.numel() != N * Sc * 4 or (jitter is not None and jitter.numel() != N):
        raise _lib.McnerfError(f"voxel_update: sig_rgb must be [N = {N}, Sc = {Sc}, 4], got {tuple(sig_rgb.shape)}")
    if z_rows is not None:
        _box.call("mcnerf_box_voxel_update_rows", grid.vox, grid.scratch, *grid.geom, *voxel_blend(beta), rays_o, rays_d,
                  z_rows, N, Sc, idx, count, int(max_rows), sig_rgb, _stream())
    else:
        _lib.call("mcnerf_voxel_update", grid.vox, grid.scratch, *grid.geom, *voxel_blend(beta), rays_o, rays_d,
                  zgrid, jitter, N, Sc, idx, count, int(max_rows), sig_rgb, _stream())


def voxel_box(grid: VoxelGrid, thresh: float, margin: int, outer, cells: Optional[Tensor] = None, box: Optional[Tensor] = None):
    """-> cells [8] int32, box [6] fp32, both on the device (the caller's own when given): the range of the cells with vox > thresh, padded by
    `margin` cells, as a box clamped to `outer` = (xmin, ymin, zmin, xmax, ymax, zmax); the outer box itself when no cell is occupied
    (cells[6] = 0) or the clamp leaves nothing (cells[6] = 2).  The rule: include/mcnerf_fit.h (mcnerf_fit_voxel_box).  One pass over the
    grid, no host synchronisation."""
    outer = [float(v) for v in outer]
    if len(outer) != 6 or isinstance(margin, bool) or not isinstance(margin, int):
        raise _lib.McnerfError(f"voxel_box: an outer box of six numbers and an integer margin, got {outer!r} and {margin!r}")
    dev = grid.vox.device
    cells = torch.empty(8, dtype=torch.int32, device=dev) if cells is None else cells
    box = torch.empty(6, dtype=torch.float32, device=dev) if box is None else box
    if cells.numel() != 8 or box.numel() != 6 or grid.vox.numel() != grid.G ** 3:
        raise _lib.McnerfError(f"voxel_box: vox [G,G,G], cells [8] and box [6], got {tuple(grid.vox.shape)}, {tuple(cells.shape)} and {tuple(box.shape)}")
    _fit.call("mcnerf_fit_voxel_box", grid.vox, grid.G, grid.bmin, grid.h, float(thresh), margin, *outer, cells, box, _stream())
    return cells, box


def voxel_query(grid: VoxelGrid, xyz: Tensor) -> Tensor:
    """query_sigma (model/mc_nerf.py:859-862): xyz [M,3] -> the cells' sigma [M]."""
    M = xyz.shape[0]
    out = torch.empty(M, dtype=torch.float32, device=xyz.device)
    _lib.call("mcnerf_voxel_query", grid.vox, *grid.geom, xyz, M, out, _stream())
    return out


def voxel_update_points(grid: VoxelGrid, xyz: Tensor, sigma: Tensor, beta: float) -> None:
    """update_sigma (model/mc_nerf.py:864-867): the update rule on explicit points xyz [M,3] with sigma [M]."""
    M = xyz.shape[0]
    if sigma.numel() != M:
        raise _lib.McnerfError(f"voxel_update_points: xyz [M,3] {tuple(xyz.shape)}, sigma [M] {tuple(sigma.shape)}")
    _lib.call("mcnerf_voxel_update_points", grid.vox, grid.scratch, *grid.geom, *voxel_blend(beta), xyz, sigma,
              M, _stream())


# --------------------------------------------------------------------------- error-guided pixel sampling (include/mcnerf.h: mcnerf_errmap_*)
class ErrorMap:
    """The three device buffers of `pixel_sampler = "error"` and the map's geometry: err [C,Th,Tw] fp32 (running squared colour error
    per tile of tile x tile pixels, Th = ceil(H / tile), Tw = ceil(W / tile), edge tiles smaller; filled with 1.0 -- optimistic: a tile
    nobody has drawn from outranks every trained tile until it is visited), scratch [C,Th,Tw] int32 (the update kernels' uint32 words,
    all zero between calls), cdf [MULTICAM_MAXSEG, Th*Tw] int64 (the sampler's workspace: always all 64 rows, 512 bytes per tile --
    1.3 MB at 800 x 800 with tile 16, 327 MB with tile 1)."""

    def __init__(self, C: int, H: int, W: int, tile: int, device):
        self.C, self.H, self.W, self.tile = int(C), int(H), int(W), int(tile)
        if self.C < 1 or self.H < 1 or self.W < 1 or self.tile < 1 or self.H * self.W > ERRMAP_MAX_PIXELS:
            raise _lib.McnerfError(f"ErrorMap needs C, H, W, tile >= 1 and H * W <= 2^26, got C = {C}, H = {H}, W = {W}, tile = {tile}")
        self.Th, self.Tw = -(-self.H // self.tile), -(-self.W // self.tile)
        self.err = torch.full((self.C, self.Th, self.Tw), 1.0, dtype=torch.float32, device=device)
        self.scratch = torch.zeros((self.C, self.Th, self.Tw), dtype=torch.int32, device=device)
        self.cdf = torch.empty((MULTICAM_MAXSEG, self.Th * self.Tw), dtype=torch.int64, device=device)

    @property
    def geom(self):
        return self.C, self.H, self.W, self.tile


def errmap_sample(emap: ErrorMap, seg_cam, seg_start, uniform_frac: float, u: Optional[Tensor] = None) -> Tensor:
    """-> pix [n] int64 in [0, H * W): the first int(uniform_frac * n_k) rays of segment k = rays [seg_start[k], seg_start[k+1]) of
    camera seg_cam[k] uniform over the image, the others with density proportional to the camera's clamped tile errors (tile by an
    integer CDF, then uniform inside the tile).  With replacement.  `u` [n,2] fp32 are the draws (torch.rand from the device generator
    when not given).  Two launches, no host synchronisation."""
    cams, start, K, n = _seg_arrays(seg_cam, seg_start)
    dev = emap.err.device
    if u is None and emap.err.is_cuda:
        u = torch.rand(n, 2, dtype=torch.float32, device=dev)
    if u is not None and u.numel() != 2 * n:
        raise _lib.McnerfError(f"errmap_sample: u must be [seg_start[-1] = {n}, 2], got {tuple(u.shape)}")
    pix = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.call("mcnerf_errmap_sample", emap.err, *emap.geom, cams, start, K, n, float(uniform_frac), u, emap.cdf,
              pix, _stream())
    return pix


def errmap_update(emap: ErrorMap, seg_cam, seg_start, pix: Tensor, rgb: Tensor, gt: Tensor, beta: float) -> None:
    """Per tile touched by the rays (pix [n] of the segments' cameras, rgb / gt [n,3]): E <- (1 - beta) E + beta max(mean squared
    colour error of a ray in the tile), deterministic in the order of arrival; rays with a non-finite error or a pixel outside the
    image are skipped, other tiles keep their bits, emap.scratch is all zero again afterwards.  Two launches."""
    cams, start, K, n = _seg_arrays(seg_cam, seg_start)
    if pix.numel() != n or rgb.numel() != 3 * n or gt.numel() != 3 * n:
        raise _lib.McnerfError(f"errmap_update: pix / rgb / gt must hold seg_start[-1] = {n} rays, got {tuple(pix.shape)}, {tuple(rgb.shape)}, {tuple(gt.shape)}")
    _lib.call("mcnerf_errmap_update", emap.err, emap.scratch, *emap.geom, cams, start, K, n, pix,
              rgb, gt, *voxel_blend(beta), _stream())


def cap_gather(idx: Tensor, perm: Tensor, keep: int):
    idx2 = torch.empty(keep, 2, dtype=torch.int32, device=idx.device)
    count = torch.empty(1, dtype=torch.int32, device=idx.device)
    _lib.call("mcnerf_cap_gather", idx, perm, int(keep), idx2,
              count, _stream())
    return idx2, count


def cap_random(idx: Tensor, count: Tensor, max_rows: int, keep: int, seed: Tensor, ws: Optional[Tensor] = None,
               out: Optional[Tensor] = None):
    """Device-side random cap (model/mc_nerf.py:630-632 without the host sync): -> idx2 [keep,2], count2 = min(count, keep).
    `ws`: the caller's own scratch of mcnerf_cap_ws_words() int32 words (whatever it holds; the call clears it first); `out`: the
    caller's own [keep,2] list buffer (rows beyond count2 are left as they are)."""
    dev = idx.device
    n_ws = int(_lib.lib().mcnerf_cap_ws_words())
    if ws is not None and ws.numel() < n_ws:
        raise _lib.McnerfError(f"cap_random: ws must hold {n_ws} words, got {tuple(ws.shape)}")
    if out is not None and out.numel() < keep * 2:
        raise _lib.McnerfError(f"cap_random: out must hold keep = {keep} pairs, got {tuple(out.shape)}")
    idx2 = torch.empty(keep, 2, dtype=torch.int32, device=dev) if out is None else out
    count2 = torch.empty(1, dtype=torch.int32, device=dev)
    if ws is None:
        ws = torch.empty(n_ws, dtype=torch.int32, device=dev)
    _lib.call("mcnerf_cap_random", idx, count, int(max_rows), int(keep), seed,
              ws, idx2, count2, _stream())
    return idx2, count2


def camera_fwd(wpose: Tensor, wpose_intr: Tensor, wfx: Tensor, wfy: Tensor, wux: Tensor, wuy: Tensor, H: int, W: int,
               wpts_intr: Optional[Tensor] = None, wpts_extr: Optional[Tensor] = None):
    """-> K [C,3,3], Kinv [C,3,3], pose [C,3,4], calib_pose [C,3,4], pix_intr [C,P,2] | None, pix_extr [C,P,2] | None
    (pixels of the calibration points wpts_* [C,P,3] through (K, calib) / (K, pose))."""
    C, dev = wpose.shape[0], wpose.device
    K = torch.empty(C, 3, 3, dtype=torch.float32, device=dev)
    Kinv = torch.empty_like(K)
    pose = torch.empty(C, 3, 4, dtype=torch.float32, device=dev)
    calib = torch.empty_like(pose)
    P = 0
    for w in (wpts_intr, wpts_extr):
        if w is not None:
            P = w.shape[1]
    pi = torch.empty(C, P, 2, dtype=torch.float32, device=dev) if wpts_intr is not None else None
    pe = torch.empty(C, P, 2, dtype=torch.float32, device=dev) if wpts_extr is not None else None
    _lib.call("mcnerf_camera_fwd", wpose, wpose_intr, wfx, wfy, wux, wuy, C, int(H), int(W),
              K, Kinv, pose, calib, wpts_intr, wpts_extr, int(P), pi, pe, _stream())
    return K, Kinv, pose, calib, pi, pe


def camera_bwd(wpose, wpose_intr, wfx, wfy, wux, wuy, H: int, W: int, dK, dKinv, dpose, dcalib,
               wpts_intr=None, wpts_extr=None, dpix_intr=None, dpix_extr=None):
    C = wpose.shape[0]
    outs = [torch.empty_like(t) for t in (wpose, wpose_intr, wfx, wfy, wux, wuy)]
    c = lambda t: None if t is None else t.contiguous()
    dK, dKinv, dpose, dcalib, dpix_intr, dpix_extr = c(dK), c(dKinv), c(dpose), c(dcalib), c(dpix_intr), c(dpix_extr)
    P = 0
    for w in (wpts_intr, wpts_extr):
        if w is not None:
            P = w.shape[1]
    _lib.call("mcnerf_camera_bwd", wpose, wpose_intr, wfx, wfy, wux, wuy, C, int(H), int(W),
              dK, dKinv, dpose, dcalib, wpts_intr, wpts_extr, int(P), dpix_intr, dpix_extr,
              *outs, _stream())
    return outs


def reproj_loss_fwd(pd: Tensor, gt: Tensor, H: int, W: int) -> Tensor:
    loss = torch.empty((), dtype=torch.float32, device=pd.device)
    _lib.call("mcnerf_reproj_loss_fwd", pd, gt, pd.numel() // 2, int(H), int(W), loss, _stream())
    return loss


def reproj_loss_bwd(pd: Tensor, gt: Tensor, H: int, W: int, dloss: Tensor) -> Tensor:
    d = torch.empty_like(pd)
    _lib.call("mcnerf_reproj_loss_bwd", pd, gt, pd.numel() // 2, int(H), int(W), dloss, d, _stream())
    return d


def train_loss(pd: Optional[Tensor], pt_gt: Optional[Tensor], H: int, W: int, normalise: bool, rgb_c: Tensor, rgb_f: Optional[Tensor], gt: Tensor):
    """MC_NeRF_Loss.forward for the keys {"intr", "rgb"} in one launch: -> out [3] = (total, L_intr, rgb term), d_pd | None, d_c, d_f | None."""
    dev = rgb_c.device
    out = torch.zeros(TRAIN_LOSS_OUT, dtype=torch.float32, device=dev)      # [3] = the kernel's arrival counter: zero on entry (include/mcnerf.h)
    np_ = pd.numel() // 2 if pd is not None else 0
    d_pd = torch.empty_like(pd) if pd is not None else None
    d_c = torch.empty_like(rgb_c)
    d_f = torch.empty_like(rgb_f) if rgb_f is not None else None
    _lib.call("mcnerf_train_loss", pd, pt_gt, np_, int(H), int(W), int(bool(normalise)), rgb_c, rgb_f, gt, rgb_c.numel(),
              out, d_pd, d_c, d_f, _stream())
    return out[:3], d_pd, d_c, d_f


def train_loss_calib(pd: Optional[Tensor], pt_gt: Optional[Tensor], H: int, W: int, normalise: bool, rgb_c: Tensor, rgb_f: Optional[Tensor],
                     gt: Tensor, color_w: Tensor, seg_cam, seg_start, reg_lambda: float, out: Optional[Tensor] = None):
    """`train_loss` with the per-camera colour calibration `color_w` [C,6] (gain - 1, bias) of the cameras `seg_cam` whose rays are the
    segments `seg_start` (host lists; they travel as kernel arguments), in one launch: -> out [4] = (total, L_intr, L_rgb, L_reg),
    d_pd | None, d_c, d_f | None, d_color [C,6] (rows of cameras outside the table exactly zero).  `out`: a buffer of
    TRAIN_LOSS_CALIB_OUT + TRAIN_LOSS_CALIB_WS floats to re-use (its word [4], the kernel's arrival counter, zero on entry: it is
    zero again on exit); allocated and zeroed when not given."""
    cams, start, K, n = _seg_arrays(seg_cam, seg_start)
    if rgb_c.numel() != 3 * n or gt.numel() != 3 * n or (rgb_f is not None and rgb_f.numel() != 3 * n):
        raise _lib.McnerfError(f"rgb_c / rgb_f / gt must hold seg_start[-1] = {n} rays of 3 channels")
    if color_w.dim() != 2 or color_w.shape[1] != 6:
        raise _lib.McnerfError(f"color_w must be [C,6], got {tuple(color_w.shape)}")
    dev = rgb_c.device
    if out is None:
        out = torch.zeros(TRAIN_LOSS_CALIB_OUT + TRAIN_LOSS_CALIB_WS, dtype=torch.float32, device=dev)
    elif out.numel() != TRAIN_LOSS_CALIB_OUT + TRAIN_LOSS_CALIB_WS:
        raise _lib.McnerfError(f"out must hold {TRAIN_LOSS_CALIB_OUT + TRAIN_LOSS_CALIB_WS} floats")
    np_ = pd.numel() // 2 if pd is not None else 0
    d_pd = torch.empty_like(pd) if pd is not None else None
    d_c = torch.empty_like(rgb_c)
    d_f = torch.empty_like(rgb_f) if rgb_f is not None else None
    d_color = torch.empty_like(color_w)
    _lib.call("mcnerf_train_loss_calib", pd, pt_gt, np_, int(H), int(W), int(bool(normalise)), rgb_c, rgb_f, gt, n,
              color_w, int(color_w.shape[0]), cams, start, K, float(reg_lambda), out, d_pd, d_c, d_f, d_color,
              out[TRAIN_LOSS_CALIB_OUT:], _stream())
    return out[:4], d_pd, d_c, d_f, d_color


def scale3_(a: Optional[Tensor], b: Tensor, c: Optional[Tensor], g: Tensor):
    """a, b, c *= g (device scalar) in place, one launch."""
    _lib.call("mcnerf_scale3", a, a.numel() if a is not None else 0, b, b.numel(), c, c.numel() if c is not None else 0, g, _stream())


def gather_gt(image_u8: Tensor, pix: Tensor) -> Tensor:
    """image_u8 [H*W, 3|4] uint8 on the device, pix [n] int64 -> [n,3] fp32 (RGBA blended on white)."""
    n = pix.numel()
    out = torch.empty(n, 3, dtype=torch.float32, device=pix.device)
    _lib.call("mcnerf_gather_gt", image_u8, int(image_u8.shape[-1]), pix, n, out, _stream())
    return out


def alloc_grad_ws(net: Net, save: MlpSave, precision: str):
    """dy / dsh workspaces of mlp_bwd for the precision mode."""
    if is16(precision):
        return (torch.empty_like(save.act),
                torch.empty(ws_bytes_16(net, save.capacity, 3, precision), dtype=torch.uint8, device=save.act.device))
    return torch.empty_like(save.act), torch.empty_like(save.sh)


def decode_frags_16(buf: Tensor, n_slots: int, width: int, rows: int, precision: str = "f16") -> Tensor:
    """Fragment-major workspace of the register-chain modes (csrc/mcnerf_16.h, mcnerf_x3.h) -> [n_slots, rows, width] fp32
    (f16x3: hi + lo, still carrying the kernel's power-of-two scale: SPLIT_SCALE_X for activations).  Debug / test helper."""
    ks = width // 16
    if precision == "f16x3":                                    # [slot][tile][part hi / lo][k-step][h][m][j], value = hi + lo
        x2 = buf.view(torch.float16).view(n_slots, -1, 2, ks, 2, 32, 8).float()
        x = x2[:, :, 0] + x2[:, :, 1]
    else:
        dt = torch.bfloat16 if precision == "bf16" else torch.float16        # ("f16x3h": the hi planes, an f16 workspace)
        x = buf.view(dt).view(n_slots, -1, ks, 2, 32, 8)        # [slot][tile][k-step][h][m][j]
    tiles = x.shape[1]
    s_, h_, j_ = torch.meshgrid(torch.arange(ks), torch.arange(2), torch.arange(8), indexing="ij")
    chan = (16 * s_ + 8 * (j_ // 4) + 4 * h_ + (j_ % 4)).reshape(-1).to(buf.device)       # channel of (s, h, j)
    y = x.permute(0, 1, 4, 2, 3, 5).reshape(n_slots, tiles * 32, ks * 16).float()          # [slot][row][(s,h,j)]
    out = torch.empty_like(y)
    out[:, :, chan] = y
    return out[:, :rows]


def decode_masks_16(mask: Tensor, n_slots: int, width: int, rows: int) -> Tensor:
    """Lane-local ReLU bit masks of the 16-bit modes (csrc/mcnerf_16.h, mlp16_fwd.hip) -> bool [n_slots, rows, width].
    Debug / test helper.  Word iw of lane (m, h) covers output tiles 2 iw, 2 iw + 1; inside a tile's 16 bits, packed word
    i (registers 2 i, 2 i + 1) sits at bit 7 - i (+ 16 for the odd register), register r = channel 32 t + 8 (r >> 2) + 4 h + (r & 3)."""
    mw = max(1, width // 64)
    mk = mask.view(n_slots, -1, 2, 32, mw).cpu()                # [slot][tile][h][m][word]
    tiles = mk.shape[1]
    out = torch.zeros(n_slots, tiles, 32, width, dtype=torch.bool)
    for t in range(width // 32):
        for r in range(16):
            i, odd = r >> 1, r & 1
            bitpos = 8 * (t & 1) + 7 - i + 16 * odd
            bit = ((mk[..., t >> 1] >> bitpos) & 1).bool()       # [slot][tile][h][m]
            for h in range(2):
                out[:, :, :, 32 * t + 8 * (r >> 2) + 4 * h + (r & 3)] = bit[:, :, h, :]
    return out.reshape(n_slots, tiles * 32, width)[:, :rows]


SPLIT_SCALE_X = 8.0      # MCNX3_SX of csrc/mcnerf_x3.h


def decode_sh_x3(buf: Tensor, rows: int) -> Tensor:
    """sh.2 outputs saved by the f16x3 forward (the fp32 accumulator tile: [tile][q][lane = 32 h + m][4]) -> [rows, 32]:
    register 4 q + e of lane (m, h) is SH row 8 q + 4 h + e.  Debug / test helper."""
    x = buf.view(torch.float32).view(-1, 4, 2, 32, 4)            # [tile][q][h][m][e]
    return x.permute(0, 3, 1, 2, 4).reshape(-1, 32)[:rows]       # [tile, m][q, h, e] -> row 8 q + 4 h + e
