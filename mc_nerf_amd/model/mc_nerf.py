"""MI355X-native counterparts of the reference's ``model/mc_nerf.py`` classes.

``MC_Model`` / ``NeRF_Model`` keep the reference's constructor (`sys_param` dict), call signatures,
attribute names, parameter names and checkpoint format, so the reference's
``main.py`` train / demo loop can drive them unchanged; the volumetric rendering underneath is the
HIP path of ``libmcnerf.so`` (no eager ATen ops, no host syncs on the train path for configs where
the 128-per-ray cap cannot bind).

Reference line numbers below are into the reference's ``model/mc_nerf.py`` unless stated otherwise.
"""
from __future__ import annotations

import logging
import os
import time
from pathlib import Path
from typing import Optional

import torch
import torch.nn as nn
import torch.distributed as dist

from .. import ops
from ..data import DeviceImageSet
from ..lens import distort_pixels, lens_model_setting
from .loss import color_calib_settings, depth_weight_setting, dist_weight_setting, mask_weight_setting
from .net_block import CorseFine_NeRF, SinCosEmbedding
from .render import CameraFn, RayBatchFn, RaygenFn, Rays, RenderCall, RenderSettings, RenderTrainFn, SamplePass, _pool, render_test, run_pass


def _rank():
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _int_key(sys_param, key, default, lo, hi=None, text=None):
    """sys_param[key] (`default` without one) when it is an integer, not a bool, in [lo, hi]; else a ValueError that names the key."""
    v = sys_param.get(key, default)
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{key} must be an integer {text or (f'>= {lo}' if hi is None else f'in [{lo}, {hi}]')}, got {v!r}")
    return v


def _number_key(sys_param, key, default, finite):
    """sys_param[key] (`default` without one) when it is an int or a float, not a bool and not NaN, and with `finite` not an
    infinity; else a ValueError that names the key."""
    v = sys_param.get(key, default)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or (finite and v in (float("inf"), float("-inf"))):
        raise ValueError(f"{key} must be a {'finite ' if finite else ''}number, got {v!r}")
    return v


# ============================================================================ renderer
class NeRF_Model(nn.Module):
    """Renderer (reference :543-867).  forward(rays_d, rays_o, epoch, step_r) -> (rgb_c, rgb_f) in
    training mode, forward(rays_d, rays_o) -> (rgb, depth, opacity) otherwise (:586-596)."""

    def __init__(self, sys_param):
        logging.info("Creating NeRF Model (HIP / gfx950)...")
        super().__init__()
        self.sys_param = sys_param
        self.mode = sys_param["mode"]
        self.device = sys_param["device_type"]
        self.near = sys_param["near"]
        self.far = sys_param["far"]
        self.samples_c = sys_param["samples"]
        self.sample_scale = sys_param["scale"]
        self.samples_f = self.samples_c * self.sample_scale
        self.dim_sh = 3 * (sys_param["MLP_deg"] + 1) ** 2
        self.white_back = sys_param["white_back"]
        self.weights_pth = sys_param.get("root_weight", "./weights")
        self.train_img_pth = sys_param.get("demo_render_pth", "./results")
        self.batch_test = sys_param["batch"]
        self.sigma_default = sys_param["sigma_default"]
        self.weight_thresh = sys_param["sample_weight_thresh"]
        self.render_h = sys_param.get("res_h", 800)
        self.render_w = sys_param.get("res_w", 800)
        self.data_name = sys_param.get("data_name", "scene")
        # identical to the reference's grids (:570-571): fp32 torch.linspace on the target device
        self.z_vals_c = torch.linspace(self.near, self.far, self.samples_c, device=self.device)
        self.z_vals_f = torch.linspace(self.near, self.far, self.samples_f, device=self.device)
        self.global_step = 0
        self.emmbedding_xyz = SinCosEmbedding(sys_param)
        self.nerf_coarse = CorseFine_NeRF(sys_param, type="coarse")
        self.nerf_fine = CorseFine_NeRF(sys_param, type="fine")
        # "precision" is this build's own sys_param key (absent in the reference's config): "f32" or "f16x3"
        self.precision = sys_param.get("precision", "f32")
        if self.precision not in ops.PRECISIONS:
            raise ValueError(f"precision must be one of {ops.PRECISIONS}")
        if self.precision != "f32" and (self.nerf_coarse.net.fp32_only or self.nerf_fine.net.fp32_only):
            raise ValueError("a net with more than one skip layer or SH degree 3 runs in precision 'f32' only "
                             f"(the register-chain kernels of '{self.precision}' take one skip layer and MLP_deg <= 2)")
        # "fine_sampler" / "n_importance" are this build's own sys_param keys as well: the fine pass's sampler, "threshold" (the
        # reference's weight-threshold refinement, :613-632; the default) or "pdf" (inverse-CDF hierarchical sampling of
        # n_importance depths per ray from the coarse weights, the fine net evaluated on the Sc + n_importance sorted depths)
        self.fine_sampler = sys_param.get("fine_sampler", "threshold")
        if self.fine_sampler not in ("threshold", "pdf"):
            raise ValueError(f"fine_sampler must be 'threshold' or 'pdf', got {self.fine_sampler!r}")
        self.n_importance = _int_key(sys_param, "n_importance", 128, 1)
        if self.fine_sampler == "pdf" and not (self.samples_c >= 3 and self.samples_c + self.n_importance <= ops.PDF_MAX_SAMPLES):
            raise ValueError(f"fine_sampler 'pdf' needs samples >= 3 and samples + n_importance <= {ops.PDF_MAX_SAMPLES}, "
                             f"got samples = {self.samples_c}, n_importance = {self.n_importance}")
        # "coarse_sampler" is this build's own key too: "dense" (the reference's coarse pass on the whole [N, samples] grid; the default)
        # or "voxel" (the coarse net on the samples in occupied cells of a [grid_nerf]^3 grid of running raw sigmas over
        # [boader_min, boader_max]^3 -- the cache the reference sketches in query_sigma / update_sigma, :859-867, and never allocates).
        # "voxel_beta" / "voxel_thresh" / "voxel_warmup_epoch" and the reference's grid keys are read and validated in "voxel" mode only.
        self.coarse_sampler = sys_param.get("coarse_sampler", "dense")
        if self.coarse_sampler not in ("dense", "voxel"):
            raise ValueError(f"coarse_sampler must be 'dense' or 'voxel', got {self.coarse_sampler!r}")
        self._voxels = None               # ops.VoxelGrid, allocated on first use ("voxel" mode only): not a parameter, not a buffer
        voxel_kw = self._voxel_settings(sys_param) if self.coarse_sampler == "voxel" else {}
        self.settings = RenderSettings(self.samples_c, self.sample_scale, float(self.weight_thresh),
                                       float(self.sigma_default), bool(self.white_back), precision=self.precision,
                                       fine_sampler=self.fine_sampler, n_importance=int(self.n_importance),
                                       coarse_sampler=self.coarse_sampler, **voxel_kw)
        # "mask_weight" is this build's own key as well: lambda > 0 makes each pass's front weight -- the rgb composite's
        # weights in front of the far-plane sample -- one more differentiable output of the train render, kept for the loss in
        # `last_front_weight`; 0.0 (the default) is today's path: the extension library is not even loaded
        self.mask_weight = mask_weight_setting(sys_param)
        self.last_front_weight = None     # mask mode: (fg_c, fg_f | None) [N] of the last train render, attached to its graph
        # "dist_weight" is this build's own key too: lambda > 0 makes each pass's distortion term -- mip-NeRF 360's, on the
        # rgb composite's weights over the normalised depths -- one more differentiable output of the train render, kept for the loss in
        # `last_distortion`; 0.0 (the default) is today's path: the regulariser library is not even loaded
        self.dist_weight = dist_weight_setting(sys_param)
        self.last_distortion = None       # distortion mode: (dist_c, dist_f | None) [N] of the last train render, attached to its graph
        # "depth_weight" is this build's own key too: lambda > 0 makes each pass's expected depth -- sum w z on the rgb
        # composite's weights, the far-plane sample included -- one more differentiable output of the train render, kept for the loss in
        # `last_expected_depth`; 0.0 (the default) is today's path: the geometry library is not even loaded
        self.depth_weight = depth_weight_setting(sys_param)
        self.settings.want_zexp = self.depth_weight > 0.0
        self.last_expected_depth = None   # depth mode: (zexp_c, zexp_f | None) [N] of the last train render, attached to its graph
        # "ray_bounds" is this build's own key too: "global" (every ray on linspace(near, far); the default and today's path:
        # nothing is allocated, the bounds library is not even loaded) or "aabb" (every ray on the part of [near, far] inside the scene
        # box "ray_bounds_box", by default the cube [boader_min, boader_max]^3 of the voxel cache)
        self.ray_bounds = sys_param.get("ray_bounds", "global")
        if self.ray_bounds not in ("global", "aabb"):
            raise ValueError(f"ray_bounds must be 'global' or 'aabb', got {self.ray_bounds!r}")
        if self.ray_bounds == "aabb":
            self.settings.ray_bounds, self.settings.box = "aabb", self._bounds_box(sys_param)
            # "ray_bounds_miss" is this build's own key too, read in "aabb" mode only, as the box: "sample" (a ray that
            # misses the box is sampled on [near, far]; the default and today's path: the hit library is not even loaded) or "skip"
            # (neither net evaluates a sample of such a ray: its rows are the prefill, its gradients exact zeros)
            self.settings.ray_bounds_miss = sys_param.get("ray_bounds_miss", "sample")
            if self.settings.ray_bounds_miss not in ("sample", "skip"):
                raise ValueError(f"ray_bounds_miss must be 'sample' or 'skip', got {self.settings.ray_bounds_miss!r}")
            # "ray_bounds_fit" and its two integers are this build's own keys too, read in "aabb" mode only: "fixed" (the box
            # is the one above; the default and today's path: the fit library is not even loaded) or "voxel" (the box is fitted on the
            # device to the occupied cells of the voxel sigma cache and refitted as training empties cells; the box above is the OUTER box)
            self.settings.ray_bounds_fit = sys_param.get("ray_bounds_fit", "fixed")
            if self.settings.ray_bounds_fit not in ("fixed", "voxel"):
                raise ValueError(f"ray_bounds_fit must be 'fixed' or 'voxel', got {self.settings.ray_bounds_fit!r}")
            if self.settings.ray_bounds_fit == "voxel" and self.coarse_sampler != "voxel":
                raise ValueError(f"ray_bounds_fit = 'voxel' needs coarse_sampler = 'voxel' (the box is fitted to its sigma grid), got {self.coarse_sampler!r}")
            self.settings.ray_bounds_fit_margin = _int_key(sys_param, "ray_bounds_fit_margin", 2, 0)
            self.settings.ray_bounds_fit_every = _int_key(sys_param, "ray_bounds_fit_every", 16, 1)
        self._scene = None                # fit mode: (scene_cells [8] int32, scene_box [6] fp32) on the device, allocated on first use: not parameters, not buffers
        self._fit_calls = 0               # fit mode: train calls past the warm-up so far (a host counter: every ray_bounds_fit_every-th refits)
        self.last_scene_box = None        # fit mode: the box tensor in force at the last render
        self.last_ray_span = None         # "aabb" mode: (lo, hi) [N,2] of the last render's rays; (near, far) on a ray the box does not clip
        self.last_ray_hit = None          # "skip" mode: [N] int32 of the last render's rays, 1 iff the box clips the ray
        self.last_coarse_selection = None  # (idx_c, count_c) of the last listed coarse pass (pruned, or "skip" mode); else None
        self.last_selection = None        # (idx, count) of the last listed fine pass ("threshold" mode, or "skip" mode); else None
        self.last_z_all = None            # the fine pass's depth rows [N, samples + n_importance] in "pdf" mode
        self.last_flat_grads = None
        self.grad_arena = None            # set per step by distributed.FlatGradSync.prepare()
        self.grad_arena_used = False
        self.ws_pool = None               # render.WorkspacePool: the kernels' saved-operand / gradient workspaces, re-used from step to step
        if self.mode != 0:
            self.nerf_ckpt_name = sys_param["demo_ckpt"]
            ckpt = torch.load(Path(self.nerf_ckpt_name), map_location=self.device)
            self.nerf_coarse.load_state_dict(self.rewrite_nerf_ckpt(ckpt, coarse=True))
            self.nerf_fine.load_state_dict(self.rewrite_nerf_ckpt(ckpt))
            logging.info("Loading weights:{}".format(self.nerf_ckpt_name))
            if self.coarse_sampler == "voxel":          # the grid is not in the checkpoint: built from the loaded coarse net
                self.rebuild_voxels()
                if self.settings.fit_box:               # ... and the box from the grid, once: render calls never refit
                    self.refit_scene_box()

    # ------------------------------------------------------------------ voxel sigma cache (:859-867)
    def _voxel_settings(self, sys_param):
        """Reads and validates the keys of "voxel" mode (a ValueError names the key) -> the RenderSettings fields."""
        number = lambda key, default: _number_key(sys_param, key, default, finite=True)
        G = _int_key(sys_param, "grid_nerf", None, 2, ops.VOXEL_MAX_G)
        bmin, bmax = number("boader_min", None), number("boader_max", None)
        if not bmin < bmax:
            raise ValueError(f"boader_min must be below boader_max, got {bmin!r} and {bmax!r}")
        self.grid_nerf, self.boader_min, self.boader_max = G, float(bmin), float(bmax)
        self.sigma_init = float(number("sigma_init", None))
        beta = number("voxel_beta", 0.1)
        if not 0.0 < beta <= 1.0:
            raise ValueError(f"voxel_beta must be in (0, 1], got {beta!r}")
        thresh = number("voxel_thresh", 0.0)
        return dict(voxel_beta=float(beta), voxel_thresh=float(thresh), voxel_warmup_epoch=_int_key(sys_param, "voxel_warmup_epoch", 1, 0))

    @staticmethod
    def _bounds_box(sys_param):
        """Reads and validates the box of "aabb" mode (a ValueError names the key) -> (xmin, ymin, zmin, xmax, ymax, zmax) as fp32 values."""
        if "ray_bounds_box" in sys_param:
            box = sys_param["ray_bounds_box"]
            if isinstance(box, (str, bytes)) or not hasattr(box, "__len__") or len(box) != 6:
                raise ValueError(f"ray_bounds_box must be six numbers (xmin, ymin, zmin, xmax, ymax, zmax), got {box!r}")
            box = [_number_key({"ray_bounds_box": v}, "ray_bounds_box", None, finite=True) for v in box]
        else:
            for key in ("boader_min", "boader_max"):
                if key not in sys_param:
                    raise ValueError(f"ray_bounds = 'aabb' needs ray_bounds_box or the cube of boader_min / boader_max: {key} is missing")
            bmin, bmax = (_number_key(sys_param, key, None, finite=True) for key in ("boader_min", "boader_max"))
            if not bmin < bmax:
                raise ValueError(f"boader_min must be below boader_max, got {bmin!r} and {bmax!r}")
            box = [bmin] * 3 + [bmax] * 3
        box = tuple(float(torch.tensor(float(v), dtype=torch.float32)) for v in box)
        if not all(v == v and abs(v) != float("inf") for v in box) or not all(lo < hi for lo, hi in zip(box[:3], box[3:])):
            raise ValueError(f"ray_bounds_box: every min must be below its max, as fp32 values, got {box!r}")
        return box

    def voxel_grid(self) -> ops.VoxelGrid:
        """The cache's two grids (allocated and filled with `sigma_init` on first use; each rank has its own)."""
        if self.coarse_sampler != "voxel":
            raise ops._lib.McnerfError("the voxel sigma cache exists in coarse_sampler = 'voxel' mode only")
        if self._voxels is None:
            self._voxels = ops.VoxelGrid(self.grid_nerf, self.boader_min, self.boader_max, self.sigma_init, self.z_vals_c.device)
        return self._voxels

    # ------------------------------------------------------------------ the scene box fitted to the cache
    def scene_buffers(self):
        """(scene_cells [8] int32, scene_box [6] fp32) of `ray_bounds_fit` = "voxel" mode, in ops.voxel_box's order, on the grid's device
        (allocated on first use; each rank has its own).  Until the first fit the box is the outer box, `settings.box`, and the cells say
        "nothing fitted" (status 0)."""
        if not self.settings.fit_box:
            raise ops._lib.McnerfError("the fitted scene box exists in ray_bounds_fit = 'voxel' mode only")
        if self._scene is None:
            dev, G = self.z_vals_c.device, self.grid_nerf
            self._scene = (torch.tensor([G, G, G, -1, -1, -1, 0, 0], dtype=torch.int32, device=dev),
                           torch.tensor(self.settings.box, dtype=torch.float32, device=dev))
        return self._scene

    @property
    def scene_box(self) -> Optional[torch.Tensor]:
        return self.scene_buffers()[1] if self.settings.fit_box else None

    @property
    def scene_cells(self) -> Optional[torch.Tensor]:
        return self.scene_buffers()[0] if self.settings.fit_box else None

    def refit_scene_box(self) -> torch.Tensor:
        """Fits the box to the grid as it is now (ops.voxel_box, in place: the tensor every later render reads) -> scene_box.  No host
        synchronisation.  Train calls do this by themselves every `ray_bounds_fit_every` calls past the warm-up; render calls never do."""
        st, (cells, box) = self.settings, self.scene_buffers()
        return ops.voxel_box(self.voxel_grid(), st.voxel_thresh, st.ray_bounds_fit_margin, st.box, cells, box)[1]

    def scene_box_status(self) -> int:
        """0: no cell was occupied at the last fit (or nothing has been fitted), the box is the outer box; 1: the box is a fitted one;
        2: the fit lay outside the outer box, the box is the outer box.  Reads the device: the one call of the feature that synchronises."""
        return int(self.scene_cells[6].item())

    @property
    def sigma_voxels(self) -> Optional[torch.Tensor]:
        """[grid_nerf]^3 fp32 running raw coarse sigma ("voxel" mode), None in "dense" mode."""
        return self.voxel_grid().vox if self.coarse_sampler == "voxel" else None

    def query_sigma(self, xyz):
        """Reference :859-862: xyz [M,3] -> the sigma of each point's cell [M]."""
        return ops.voxel_query(self.voxel_grid(), xyz.reshape(-1, 3).float().contiguous())

    def update_sigma(self, xyz, sigma, beta):
        """Reference :864-867, with the cache's deterministic rule: per touched cell V <- (1 - beta) V + beta max(sigma in the cell)."""
        ops.voxel_update_points(self.voxel_grid(), xyz.reshape(-1, 3).float().contiguous(), sigma.reshape(-1).float().contiguous(), beta)

    def voxel_centres(self, lo: int, hi: int, device) -> torch.Tensor:
        """Centres boader_min + (i + 1/2) (scope / G) of the cells with linear index lo .. hi-1, [hi - lo, 3] fp32."""
        G = self.grid_nerf
        axis = (torch.arange(G, dtype=torch.float32) + 0.5) * torch.tensor((self.boader_max - self.boader_min) / G, dtype=torch.float32) \
            + torch.tensor(self.boader_min, dtype=torch.float32)
        axis = axis.to(device)
        lin = torch.arange(lo, hi, dtype=torch.int64, device=device)
        return torch.stack([axis[lin // (G * G)], axis[(lin // G) % G], axis[lin % G]], -1).contiguous()

    @torch.no_grad()
    def rebuild_voxels(self, model_coarse=None, chunk: int = 1 << 19):
        """V[cell] = raw sigma of the coarse net at the cell's centre, for every cell (the demo path: the grid is not in the
        checkpoint).  Stand-alone exact-fp32 kernels (ops.encode + ops.mlp_apply) in `chunk`-cell pieces; sigma does not depend on
        the view direction, which is fixed."""
        grid = self.voxel_grid()
        model = self.nerf_coarse if model_coarse is None else model_coarse
        dev = grid.vox.device
        net, flat = model.net, model.flat_params()
        if flat.device != dev:              # (demo mode builds the grid at construction, before the caller's .to(device) moves the nets)
            flat = ops.flatten_params(net, [p.detach() for p in model.ordered_parameters()], dev)
        packed = ops.pack_weights(net, flat, precision="f32")
        barf_w = self.emmbedding_xyz.barf_weights_on(1, dev)
        total = self.grid_nerf ** 3
        dirs = torch.tensor([0.0, 0.0, 1.0], device=dev).expand(min(chunk, total), 3).contiguous()
        out = grid.vox.view(-1)
        for lo in range(0, total, chunk):
            hi = min(lo + chunk, total)
            enc = ops.encode(self.voxel_centres(lo, hi, dev), barf_w)
            out[lo:hi] = ops.mlp_apply(net, flat, packed, enc, dirs[:hi - lo])[:, 0]
        return grid.vox

    # ------------------------------------------------------------------ API (:586-596)
    def forward(self, *args):
        self.global_step += 1
        if self.mode == 0:
            rays_d, rays_o, cur_epoch, step_r = args
            rgb_c, rgb_f = self.render_rays_train(rays_d, rays_o, cur_epoch, step_r, only_coarse=False)
            return rgb_c, rgb_f
        rays_d, rays_o = args
        return self.render_rays_test(rays_d, rays_o, self.nerf_coarse, self.nerf_fine)

    def _dev(self, t):
        return t.to(device=self.z_vals_c.device, dtype=torch.float32)

    def _draws(self, N, dev, train, only_coarse, jitter, eps_c, eps_sel, u, eps_f):
        """The draws of one render, those not given drawn from torch's device generator in the reference's order (jitter, eps_c,
        eps_sel, u, eps_f), as fp32 tensors on the model's device.  Rendering (`train` False) has no jitter, and its `u`
        defaults to linspace(0, 1, n_importance) for every ray: a deterministic render."""
        pdf = self.settings.pdf and not only_coarse
        if train and jitter is None:
            jitter = torch.empty(N, 1, device=dev).uniform_(0.0, (self.far - self.near) / self.samples_c)
        if eps_c is None:
            eps_c = torch.randn(N, self.samples_c, device=dev)
        if not only_coarse:
            if eps_sel is None:
                eps_sel = torch.randn(N, self.samples_c, device=dev)
            if pdf and u is None:
                u = torch.rand(N, self.n_importance, device=dev) if train else torch.linspace(0.0, 1.0, self.n_importance, device=dev).expand(N, -1)
            if eps_f is None:
                eps_f = torch.randn(N, self.settings.samples_pdf if pdf else self.samples_f, device=dev)
        on = lambda t: None if t is None else self._dev(t).contiguous()
        return None if jitter is None else self._dev(jitter), on(eps_c), on(eps_sel), on(u) if pdf else None, on(eps_f)

    def render_rays_train(self, rays_d, rays_o, cur_epoch, step_r, only_coarse=False, *,
                          jitter=None, eps_c=None, eps_sel=None, eps_f=None, cap_perm=None, u=None):
        """Reference :598-646.  The keyword-only tensors are the reference's random draws
        (U(0,(far-near)/Sc) per ray; three N(0,1) tensors; the cap permutation); when omitted they are
        drawn from torch's device generator in the reference's order.  `fine_sampler = "pdf"`: `u` [N, n_importance] are the
        sampler's U(0,1) draws (drawn after eps_sel), eps_f is [N, samples + n_importance] and cap_perm is not used."""
        N, dev = rays_d.shape[0], rays_d.device
        want_fg = self.mask_weight > 0.0
        if want_fg and not rays_d.is_cuda:
            raise ops._lib.McnerfError(f"mask_weight = {self.mask_weight}: the front weight is a HIP kernel, got rays on {dev} (no CPU fallback)")
        want_dist = self.dist_weight > 0.0
        if want_dist and not rays_d.is_cuda:
            raise ops._lib.McnerfError(f"dist_weight = {self.dist_weight}: the distortion term is a HIP kernel, got rays on {dev} (no CPU fallback)")
        want_zexp = self.settings.want_zexp
        if want_zexp and not rays_d.is_cuda:
            raise ops._lib.McnerfError(f"depth_weight = {self.depth_weight}: the expected depth is a HIP kernel, got rays on {dev} (no CPU fallback)")
        if self.settings.aabb and not rays_d.is_cuda:
            raise ops._lib.McnerfError(f"ray_bounds = 'aabb': the per-ray depths are a HIP kernel, got rays on {dev} (no CPU fallback)")
        if self.settings.fit_box and cur_epoch >= self.settings.voxel_warmup_epoch:
            if self._fit_calls % self.settings.ray_bounds_fit_every == 0:
                self.refit_scene_box()
            self._fit_calls += 1
        if N == 0:                                  # empty batch: empty results (the reference's tensor ops do the same)
            self.last_expected_depth = (rays_d.new_zeros(0), None if only_coarse else rays_d.new_zeros(0)) if want_zexp else None
            e3, e1 = rays_d.new_zeros(0, 3), rays_d.new_zeros(0, 1)
            self.last_front_weight = (rays_d.new_zeros(0), None if only_coarse else rays_d.new_zeros(0)) if want_fg else None
            self.last_distortion = (rays_d.new_zeros(0), None if only_coarse else rays_d.new_zeros(0)) if want_dist else None
            return (e3, None, e1) if only_coarse else (e3, e3.clone())
        draws = self._draws(N, dev, True, only_coarse, jitter, eps_c, eps_sel, u, eps_f)
        params = self.nerf_coarse.ordered_parameters() + self.nerf_fine.ordered_parameters()
        self.nerf_coarse.flat_params()
        self.nerf_fine.flat_params()
        call = RenderCall(self, self.nerf_coarse, self.nerf_fine, step_r, only_coarse, *draws, cap_perm,
                          prune=self.settings.voxel and cur_epoch >= self.settings.voxel_warmup_epoch, want_dist=want_dist,
                          want_fg=want_fg)
        rgb_c, rgb_f, depth_c, fg_c, fg_f, dist_c, dist_f, zexp_c, zexp_f = RenderTrainFn.apply(rays_d, rays_o, call, *params)
        self.last_expected_depth = (zexp_c, zexp_f) if want_zexp else None
        self.last_front_weight = (fg_c, fg_f) if want_fg else None
        self.last_distortion = (dist_c, dist_f) if want_dist else None
        return (rgb_c, None, depth_c) if only_coarse else (rgb_c, rgb_f)

    @torch.no_grad()
    def render_rays_test(self, rays_d, rays_o, model_coarse, model_fine, *, eps_c=None, eps_sel=None, eps_f=None, _prepared=None, u=None):
        """Reference :648-680 (the nets are arguments because valid_train passes freshly loaded ones).  `fine_sampler = "pdf"`:
        `u` [N, n_importance] defaults to linspace(0, 1, n_importance) for every ray (a deterministic render) and eps_f is
        [N, samples + n_importance]."""
        N, dev = rays_d.shape[0], rays_d.device
        if self.settings.aabb and not rays_d.is_cuda:
            raise ops._lib.McnerfError(f"ray_bounds = 'aabb': the per-ray depths are a HIP kernel, got rays on {dev} (no CPU fallback)")
        if N == 0:
            return rays_d.new_zeros(0, 3), rays_d.new_zeros(0, 1), rays_d.new_zeros(0, 1)
        _, eps_c, eps_sel, u, eps_f = self._draws(N, dev, False, False, None, eps_c, eps_sel, u, eps_f)
        return render_test(self, model_coarse, model_fine, rays_d.float(), rays_o.float(), eps_c, eps_sel, eps_f, _prepared, u=u)

    def reserve_workspaces(self, n_rays: int):
        """Sizes the training workspaces of both nets for `n_rays`-ray steps now (they are re-used from step to step afterwards:
        render.WorkspacePool), so that the first timed / synchronised step of a multi-GPU run allocates nothing."""
        dev, st, pool = self.z_vals_c.device, self.settings, _pool(self)
        if st.voxel:
            self.voxel_grid()                       # (the list itself has the dense pass's capacity: the pool's keys do not change)
        if st.fit_box:
            self.scene_buffers()
        for net, rows in ((self.nerf_coarse.net, n_rays * st.samples_c), (self.nerf_fine.net, st.fine_rows(n_rays, train=True))):
            save = pool.take_save(net, rows, dev, st.precision)
            pool.give_grad(net, save, st.precision, pool.take_grad(net, save, st.precision))
            pool.give_save(net, save, st.precision)

    # ------------------------------------------------------------------ per-pass API of the reference (:682-736)
    def inference(self, model, embedding_xyz, step_r, xyz, rays_d, z_vals, idx_render=None, coarse=True, *, eps=None):
        """Reference :682-727.  Differentiable like the reference's: when autograd is recording and any input or parameter
        requires a gradient the pass runs on the stand-alone differentiable kernels (`_inference_general`: EncodeFn, MlpApplyFn,
        composites in tensor ops); otherwise on the fused forward-only path (`_inference`).

        DISPATCH, explicitly: the differentiable path is taken whenever grad mode is on and ANY of `xyz`, `rays_d`, `z_vals` or
        the net's parameters requires a gradient -- i.e. always for a training-mode model called outside `torch.no_grad()`.
        That path computes in exact fp32 whatever `precision` the model was built with, ignores `coarse`, and keeps
        (depth + 2) * rows * width floats of saved activations: it exists for API parity (a caller differentiating through
        `inference` directly), not for rendering.  Render under `torch.no_grad()` (as `render_rays_test`, `valid_train` and the
        demo path do) to get the fused kernels in the configured precision; training goes through `render_rays_train`."""
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                           for t in (xyz, rays_d, z_vals, *model.parameters())):
            return self._inference_general(model, embedding_xyz, step_r, xyz, rays_d, z_vals.float(), idx_render, eps)
        with torch.no_grad():
            return self._inference(model, embedding_xyz, step_r, xyz, rays_d, z_vals, idx_render, coarse, eps=eps)

    def _inference(self, model, embedding_xyz, step_r, xyz, rays_d, z_vals, idx_render=None, coarse=True, *, eps=None):
        """One pass of one net on given samples -> (rgb [N,3], sigmas [N,S], xyz, depth [N,1], opacity [N,1]), the
        reference's `inference` (:682-727) for callers that use it directly.

        The fused HIP kernels generate the positions themselves from (origin, direction, z grid + per-ray jitter).  When
        `z_vals` has the reference's structure (its own call sites always do): `z_vals[n, j] = grid[j] + jitter[n]` with
        `grid` this model's coarse or fine grid, that path is taken and the origins are recovered from `xyz[:, 0]`.  Any
        other `xyz` / `z_vals` goes through the stand-alone kernels on the given positions (`_inference_general`).
        Forward only (`inference` routes gradient requests to `_inference_general`).  `eps` is the N(0,1) draw of
        `sigma2weights` (drawn from the device generator when not given)."""
        N, S_ = z_vals.shape
        dev = rays_d.device
        z_vals = z_vals.float()
        structured = S_ in (self.samples_c, self.samples_f)
        if structured:
            grid = self.z_vals_c if S_ == self.samples_c else self.z_vals_f
            jitter = (z_vals[:, 0] - grid[0]).contiguous()
            structured = bool(torch.allclose(z_vals, grid.unsqueeze(0) + jitter.unsqueeze(1), atol=1e-5, rtol=0))
        if not structured:
            return self._inference_general(model, embedding_xyz, step_r, xyz, rays_d, z_vals, idx_render, eps)
        rays_d = rays_d.float().contiguous()
        rays_o = (xyz.reshape(N, S_, 3)[:, 0].float() - rays_d * z_vals[:, :1]).contiguous()
        st = self.settings
        flat = model.flat_params()
        packed = ops.pack_weights(model.net, flat, precision=st.precision)
        barf_w = embedding_xyz.barf_weights_on(step_r, dev, pad=10)
        idx = count = None
        if idx_render is None:
            out = torch.empty(N, S_, 4, dtype=torch.float32, device=dev)
        else:                                                   # scatter into the defaults (:692-694, 701)
            out = torch.ones(N, S_, 4, dtype=torch.float32, device=dev)
            out[..., 0] = st.sigma_default
            idx = idx_render.to(device=dev, dtype=torch.int32).contiguous()
            count = torch.tensor([idx.shape[0]], dtype=torch.int32, device=dev)
        if eps is None:
            eps = torch.randn(N, S_, device=dev)
        p = SamplePass(model, flat, packed, grid, jitter, None, self._dev(eps).float().contiguous(), out,
                       idx, count, 0 if idx is None else idx.shape[0])
        rgb, depth, opacity, _, _ = run_pass(p, st, Rays(rays_o, rays_d, barf_w), want_depth=True)
        return rgb, out[..., 0], xyz, depth, opacity

    def _inference_general(self, model, embedding_xyz, step_r, xyz, rays_d, z_vals, idx_render, eps):
        """`inference` on arbitrary sample positions (reference :682-727 literally): encode the given `xyz` and run the net
        with the stand-alone exact-fp32 kernels through the modules' own forwards (`SinCosEmbedding.forward`,
        `CorseFine_NeRF.forward`: differentiable when a gradient is requested), scatter into the defaults (sigma_default,
        white) when an index list is given, then both composites in tensor ops (:705-725)."""
        st = self.settings
        N, S_ = z_vals.shape
        dev = rays_d.device
        rays_d = rays_d.float()
        xyz3 = xyz.reshape(N, S_, 3).float()
        if idx_render is None:
            dirs = rays_d.unsqueeze(1).expand(-1, S_, -1).reshape(-1, 3)
            out = model(embedding_xyz(xyz3.reshape(-1, 3), step_r), dirs).reshape(N, S_, 4)
        else:
            r, j = idx_render[:, 0].long().to(dev), idx_render[:, 1].long().to(dev)
            out = torch.ones(N, S_, 4, dtype=torch.float32, device=dev)
            out[..., 0] = st.sigma_default
            if r.numel():
                raw = model(embedding_xyz(xyz3[r, j], step_r), rays_d[r])
                out = out.index_put((r, j), raw)
        if eps is None:
            eps = torch.randn(N, S_, device=dev)
        sig, rgbs = out[..., 0], out[..., 1:]
        deltas = torch.cat([z_vals[:, 1:] - z_vals[:, :-1], torch.full_like(z_vals[:, :1], 1e10)], -1)
        sd = torch.nn.functional.softplus(sig) * (deltas * rays_d.norm(dim=-1, keepdim=True))
        alpha = 1.0 - torch.exp(-sd)
        T = torch.exp(-torch.cat([torch.zeros_like(sd[:, :1]), sd[:, :-1]], 1).cumsum(1))
        prob = T * alpha
        opacity, depth = prob.sum(1, keepdim=True), (z_vals * prob).sum(1, keepdim=True)
        w = self.sigma2weights(deltas, sig, self._dev(eps).float())
        rgb = (w.unsqueeze(-1) * rgbs).sum(1)
        if st.white_back:
            rgb = rgb + 1.0 - w.sum(1, keepdim=True)
        return rgb, sig, xyz, depth, opacity

    @staticmethod
    def sigma2weights(deltas, sigmas, eps=None):
        """Reference :729-736 on arbitrary `deltas` (compatibility helper in plain tensor ops; the render path computes the
        same weights inside the fused composite kernels)."""
        if eps is None:
            eps = torch.randn_like(sigmas)
        alphas = 1.0 - torch.exp(-deltas * torch.nn.functional.softplus(sigmas + eps))
        shifted = torch.cat([torch.ones_like(alphas[:, :1]), 1.0 - alphas + 1e-10], -1)
        return alphas * torch.cumprod(shifted, -1)[:, :-1]

    # ------------------------------------------------------------------ checkpoints (:738-752, 815-837)
    def save_model(self, model, epoch):
        save_path = os.path.join(Path(self.weights_pth), Path("train"))
        os.makedirs(save_path, exist_ok=True)
        stamp = time.strftime("%Y-%m-%d-%H-%M-%S", time.localtime())
        self.model_name = "{}-EPOCH-{}-{}.ckpt".format(self.data_name, epoch, stamp)        # reference attributes (:743-744)
        self.file_path = os.path.join(save_path, self.model_name)
        self.ckpt_path = self.file_path
        if _rank() == 0:
            # `model` is what main.py passes: the (possibly DDP-wrapped) MC_Model; its state_dict() keys are the
            # checkpoint's (DDP's "module." prefix included, exactly as the reference writes them)
            torch.save({"model_nerf": model.state_dict()}, self.file_path)
            logging.info("Save model:{}".format(self.model_name))
        return self.file_path

    @staticmethod
    def rewrite_nerf_ckpt(ckpt, coarse=False):
        """{'model_nerf': MC_Model.state_dict()} -> state dict of one net: the key suffix after the `nerf_coarse` /
        `nerf_fine` path component (reference :815-837; also strips DDP's `module.` prefix that way)."""
        name = "nerf_coarse" if coarse else "nerf_fine"
        out = {}
        for k, v in ckpt["model_nerf"].items():
            parts = k.split(".")
            if name in parts:
                out[".".join(parts[parts.index(name) + 1:])] = v
        return out

    @staticmethod
    def cal_psnr(pred, gt):
        return -10.0 * torch.log10(torch.mean((pred - gt) ** 2))

    psnr_score = cal_psnr          # reference name (:839-848)

    @torch.no_grad()
    def render_chunked(self, rays_d, rays_o, model_coarse, model_fine, chunk=None):
        """render_rays_test over all rays in `chunk`-ray pieces (the demo / validation hot loop, :106-122, 778-786);
        everything stays on the device.  -> rgb [M,3], depth [M,1], opacity [M,1]"""
        chunk = chunk or self.batch_test
        M = rays_d.shape[0]
        rgb = torch.empty(M, 3, dtype=torch.float32, device=rays_d.device)
        depth = torch.empty(M, 1, dtype=torch.float32, device=rays_d.device)
        opac = torch.empty(M, 1, dtype=torch.float32, device=rays_d.device)
        # the weights are constant inside the loop: re-layout them (and upload the BARF weights) once per image, not per chunk
        prec = self.settings.precision
        prepared = None
        if M > 0:
            prepared = (ops.pack_weights(model_coarse.net, model_coarse.flat_params(), precision=prec),
                        ops.pack_weights(model_fine.net, model_fine.flat_params(), precision=prec),
                        self.emmbedding_xyz.barf_weights_on(1, rays_d.device, pad=10))
        for i in range(0, M, chunk):
            r, d, o = self.render_rays_test(rays_d[i:i + chunk], rays_o[i:i + chunk], model_coarse, model_fine, _prepared=prepared)
            rgb[i:i + chunk], depth[i:i + chunk], opac[i:i + chunk] = r, d, o
        return rgb, depth, opac

    @torch.no_grad()
    def valid_train(self, epoch, val_data, epoch_type):
        """Reference :754-813: on rank 0 re-load the checkpoint just written by save_model into fresh nets, render the
        validation view in `batch` chunks, write the image / ground truth / depth PNGs and log the PSNR (computed on the
        device; SSIM / LPIPS are third-party metrics outside the hot path); the other ranks wait at the barrier.
        Returns 0 in the camera-only stage, None otherwise (as the reference); the render is kept in
        `self.last_validation` = dict(rgb, depth, psnr) for callers that want it."""
        if epoch_type in ["CAM_PARAM_EPOCH"]:
            return 0
        if _rank() == 0:
            rays_d, rays_o, gt_rgbs = val_data
            ckpt = torch.load(self.file_path, map_location=self.device)
            logging.info("Loading model: {}".format(self.model_name))
            val_c = CorseFine_NeRF(self.sys_param, type="coarse").to(self.device)
            val_f = CorseFine_NeRF(self.sys_param, type="fine").to(self.device)
            val_c.load_state_dict(self.rewrite_nerf_ckpt(ckpt, coarse=True))
            val_f.load_state_dict(self.rewrite_nerf_ckpt(ckpt, coarse=False))
            val_c.eval(), val_f.eval()
            rgb, depth, _ = self.render_chunked(rays_d, rays_o, val_c, val_f)
            gt = gt_rgbs.reshape(-1, 3).to(rgb.device)
            psnr = self.cal_psnr(rgb, gt)
            self.last_validation = {"rgb": rgb, "depth": depth, "psnr": psnr}
            logging.info("PSNR:{}".format(float(psnr)))
            if rgb.shape[0] == self.render_h * self.render_w:
                self._save_validation_images(epoch, rgb, gt, depth)
        if dist.is_available() and dist.is_initialized():
            dist.barrier()
        return None

    def _save_validation_images(self, epoch, rgb, gt, depth):
        try:
            from PIL import Image
        except ImportError:                                     # image files are a convenience, not part of the path
            return
        base = os.path.join(Path(self.train_img_pth), Path(self.data_name))
        os.makedirs(base, exist_ok=True)

        def u8(t, ch):
            return (t.reshape(self.render_h, self.render_w, ch).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
        Image.fromarray(u8(rgb, 3), "RGB").save(os.path.join(base, "epoch_{}.png".format(epoch)))
        Image.fromarray(u8(gt, 3), "RGB").save(os.path.join(base, "epoch_{}_gt.png".format(epoch)))
        Image.fromarray(u8(depth, 1)[..., 0], "L").save(os.path.join(base, "epoch_{}_depth.png".format(epoch)))


# ============================================================================ multi-camera model
class MC_Model(nn.Module):
    """Camera parametrisation + ray generation + renderer (reference :24-540).

    Train call:  model(data, epoch, epoch_type, cur_ratio) -> (loss_dict, intr_show, pose_show, rays_valid)
    Demo call:   model(img_idx) -> (rgbs, depth, opacity) on the CPU, chunked by ``batch`` (:106-122).
    """

    def __init__(self, sys_param):
        logging.info("Creating MC-NeRF Model (HIP / gfx950)...")
        super().__init__()
        self.sys_param = sys_param
        self.mode = sys_param["mode"]
        self.device = sys_param["device_type"]
        self.batch = sys_param["batch"]
        # "cams_per_step" is this build's own sys_param key (absent in the reference's config): the number K of cameras whose rays share
        # one NeRF-stage train step.  1 (the default) is the reference's step, one camera; K > 1 splits the batch into K segments of
        # consecutive rays, one camera each, through the fused ray-batch kernel (RayBatchFn)
        self.cams_per_step = _int_key(sys_param, "cams_per_step", 1, 1, min(ops.MULTICAM_MAXSEG, self.batch),
                                      f"in [1, min({ops.MULTICAM_MAXSEG}, batch = {self.batch})]")
        self.last_step_segments = None    # (camera ids, seg_start) of the last multi-camera step
        self.last_step_pix = None         # its pixel ids [batch]
        self._seg_index = None            # segment of every ray (device int64 [batch]), built once: host float stacks, error-map colours
        # "color_calib" / "color_calib_reg" are this build's own keys as well: "none" (the default: today's path, no
        # parameter) or "affine" -- one more parameter weights_color [C,6], camera c is modelled to observe
        # (1 + weights_color[c, 0:3]) * rgb + weights_color[c, 3:6] of the rendered colour, fused into the NeRF stages' loss
        self.color_calib, self.color_calib_reg = color_calib_settings(sys_param)
        # "pixel_sampler" is this build's own key too: "uniform" (the default: today's draw, nothing allocated) or "error"
        # -- the NeRF stages draw their pixels in proportion to a running per-tile colour error (ops.ErrorMap).  "error_tile" /
        # "error_beta" / "error_uniform_frac" are read and validated in "error" mode only; their defaults are starting values, not tuned
        # (the map's CDF workspace is 512 bytes per tile whatever cams_per_step is: a small error_tile on a large image costs memory)
        self.pixel_sampler = sys_param.get("pixel_sampler", "uniform")
        if not isinstance(self.pixel_sampler, str) or self.pixel_sampler not in ("uniform", "error"):
            raise ValueError(f"pixel_sampler must be 'uniform' or 'error', got {self.pixel_sampler!r}")
        # "lens_model" is this build's own key as well: "pinhole" (the default: today's path, no parameter) or "radial" --
        # one more parameter weights_lens [C,2] = (k1, k2) per training camera, OpenCV's two-coefficient radial model, undistorted inside
        # the NeRF stages' ray kernel (RayBatchFn with its lens input) and applied in closed form to the calibration-tag reprojection
        self.lens_model = lens_model_setting(sys_param)
        # "mask_weight" is this build's own key too: lambda > 0 adds the alpha-mask term of the renderer's front weights
        # to the NeRF stages' loss, the alpha of the drawn pixels gathered from the device-resident RGBA images; no parameter
        self.mask_weight = mask_weight_setting(sys_param)
        # "dist_weight" likewise: lambda > 0 adds the distortion term of the renderer's two passes to the NeRF stages'
        # loss; no parameter, no extra data
        self.dist_weight = dist_weight_setting(sys_param)
        # "depth_weight" likewise: lambda > 0 adds the depth term of the renderer's two expected depths to the NeRF
        # stages' loss, the targets of the drawn pixels gathered from the image set's device-resident depth; no parameter
        self.depth_weight = depth_weight_setting(sys_param)
        self._error_map = None            # ops.ErrorMap, allocated on first use ("error" mode only): not a parameter, not a buffer
        if self.pixel_sampler == "error":
            self.error_tile, self.error_beta, self.error_uniform_frac = self._error_settings(sys_param)
        self.intr = sys_param["intr_mat"]
        self.intr_inv = sys_param["intr_mat_inv"]
        # the constant intrinsics live on the device from the start (a per-step .to(device) of a host tensor is a
        # synchronous copy: it would stall the host behind every queued kernel)
        self.intr_train, self.intr_test, self.intr_val = [t.to(self.device) for t in self.intr]
        self.intr_train_inv, self.intr_test_inv, self.intr_val_inv = [t.to(self.device) for t in self.intr_inv]
        self.gt_pose = sys_param["gt_pose"].to(self.device)
        self.test_pose = sys_param["test_pose"].to(self.device)
        self.valid_pose = sys_param["valid_pose"].to(self.device)
        self.valid_rgbs = sys_param["valid_rgbs"].to(self.device)
        self.img_h = sys_param["data_img_h"]
        self.img_w = sys_param["data_img_w"]
        self.data_name = sys_param.get("data_name", "scene")
        self.data_numb = sys_param["data_numb"]
        self.train_numb, self.test_numb, self.val_numb = self.data_numb
        self.register_parameters()
        self.nerf = NeRF_Model(sys_param).to(self.device)
        self.count_rays = 0
        self.intr_inv_adj = None
        self.opt_idx = 0
        self.last_epoch_type = 0

    # ------------------------------------------------------------------ parameters (:347-371)
    def register_parameters(self):
        C, dev = self.train_numb, self.device
        for name, shape in (("weights_pose", (C, 6)), ("weights_pose_intr", (C, 6)), ("weights_ux", (C,)),
                            ("weights_uy", (C,)), ("weights_fx", (C,)), ("weights_fy", (C,))):
            self.register_parameter(name, nn.Parameter(torch.ones(shape, device=dev), requires_grad=True))
        if self.color_calib == "affine":     # an offset from identity (zeros): weight decay pulls towards "no correction"
            self.register_parameter("weights_color", nn.Parameter(torch.zeros(C, 6, device=dev), requires_grad=True))
        if self.lens_model == "radial":      # an offset from "no distortion" (zeros), as weights_color
            self.register_parameter("weights_lens", nn.Parameter(torch.zeros(C, 2, device=dev), requires_grad=True))

    def optimizer_groups(self, lazy_cameras=True):
        """The two param groups of a row-lazy optimiser, each in `named_parameters` order: the radiance-field tensors,
        and every per-camera tensor registered above ([C, ...]: a row per training camera) with `"lazy_rows": lazy_cameras`, so that
        RAdam steps a camera's rows only when the camera has a gradient.  Callers add `lr` etc. to the dicts; `RAdam(model.parameters())`
        stays the dense optimiser of the reference."""
        named = list(self.named_parameters())
        return [{"params": [p for n, p in named if n.startswith("nerf.")]},
                {"params": [p for n, p in named if not n.startswith("nerf.")], "lazy_rows": bool(lazy_cameras)}]

    # ------------------------------------------------------------------ error-guided pixel sampling
    @staticmethod
    def _error_settings(sys_param):
        """Reads and validates the keys of "error" mode (a ValueError names the key) -> (error_tile, error_beta, error_uniform_frac)."""
        number = lambda key, default: float(_number_key(sys_param, key, default, finite=False))
        tile = _int_key(sys_param, "error_tile", 16, 1, 256)
        beta = number("error_beta", 0.5)
        if not 0.0 < beta <= 1.0:
            raise ValueError(f"error_beta must be in (0, 1], got {beta!r}")
        frac = number("error_uniform_frac", 0.5)
        if not 0.0 <= frac <= 1.0:
            raise ValueError(f"error_uniform_frac must be in [0, 1], got {frac!r}")
        h, w = sys_param["data_img_h"], sys_param["data_img_w"]
        if h * w > ops.ERRMAP_MAX_PIXELS:
            raise ValueError(f"pixel_sampler 'error' needs data_img_h * data_img_w <= 2^26, got {h} x {w}")
        return tile, beta, frac

    def reserve_error_map(self) -> ops.ErrorMap:
        """The map's buffers (allocated and filled with 1.0 on first use; each rank has its own, learnt from its own shard): call it
        ahead of the first step so that no timed / synchronised step allocates."""
        if self.pixel_sampler != "error":
            raise ops._lib.McnerfError("the error map exists in pixel_sampler = 'error' mode only")
        if self._error_map is None:
            self._error_map = ops.ErrorMap(self.train_numb, self.img_h, self.img_w, self.error_tile, self.weights_pose.device)
        return self._error_map

    def error_map(self, cam=None) -> torch.Tensor:
        """A detached copy of the running per-tile errors: [Th,Tw] of training camera `cam`, or [C,Th,Tw] of all of them."""
        err = self.reserve_error_map().err
        if cam is None:
            return err.detach().clone()
        return err[_int_key({"cam": cam}, "cam", None, 0, self.train_numb - 1)].detach().clone()

    def reset_error_map(self):
        """Refills the map with 1.0: every tile is unvisited again."""
        self.reserve_error_map().err.fill_(1.0)

    def draw_error_uniforms(self, n):
        """Hook of "error" mode: the [n,2] fp32 uniforms of the step's draw, or None (the default) = torch.rand from the device
        generator inside ops.errmap_sample; parity tests replace this method."""
        return None

    def _draw_error_pixels(self, cams, seg_start):
        return ops.errmap_sample(self.reserve_error_map(), cams, seg_start, self.error_uniform_frac, self.draw_error_uniforms(seg_start[-1]))

    @torch.no_grad()
    def _update_error_map(self, cams, seg_start, pix, rgb, gt):
        """The map learns the step's render: with color_calib = "affine" the colours are first corrected with the detached gain and
        bias of every ray's camera, so that the map ranks what the loss sees.  The six coefficients per ray are rows of weights_color
        picked by host camera ids (views) and spread over the segments by the device index of `ops.ray_segment_index`: the same few
        launches at any K, no host -> device copy and no host synchronisation."""
        rgb = rgb.detach()
        if self.color_calib == "affine":
            w = self.weights_color.detach()
            if len(cams) == 1:
                w = w[cams[0]]
            else:
                if self._seg_index is None:
                    self._seg_index = ops.ray_segment_index(self.batch, len(cams), rgb.device)
                w = torch.stack([w[c] for c in cams])[self._seg_index]
            rgb = (1.0 + w[..., :3]) * rgb + w[..., 3:]
        ops.errmap_update(self.reserve_error_map(), cams, seg_start, pix, rgb.contiguous(), gt.detach().float().contiguous(), self.error_beta)

    def color_correction(self):
        """(gain [C,3], bias [C,3]) of the training cameras, detached: camera c observes gain[c] * rgb + bias[c]."""
        if self.color_calib != "affine":
            raise ValueError("color_correction() needs color_calib = 'affine'")
        w = self.weights_color.detach()
        return 1.0 + w[:, :3], w[:, 3:].clone()

    # ------------------------------------------------------------------ radial lens distortion
    def lens_coefficients(self):
        """(k1, k2) of the training cameras [C,2], detached."""
        if self.lens_model != "radial":
            raise ValueError("lens_coefficients() needs lens_model = 'radial'")
        return self.weights_lens.detach().clone()

    @torch.no_grad()
    def train_camera_rays(self, cam):
        """All H*W rays (rays_d, rays_o) of training camera `cam` through its learnt pose, K and lens."""
        if self.lens_model != "radial":
            raise ValueError("train_camera_rays() needs lens_model = 'radial'")
        cam = _int_key({"cam": cam}, "cam", None, 0, self.train_numb - 1)
        keep = (self.intr_inv_adj, getattr(self, "_reproj", [None, None]))      # (a step's cached camera outputs stay as they were)
        intr_adj, pose_adj, _ = self.add_weights2param(True, True, False)
        kinv = self.intr_inv_adj if self.intr_inv_adj is not None else self.inverse_intrinsic(intr_adj)
        self.intr_inv_adj, self._reproj = keep
        npix = self.img_h * self.img_w
        if getattr(self, "_all_pix", None) is None:
            self._all_pix = torch.arange(npix, device=self.device)
        _, rays_d, rays_o, _ = ops.lens_ray_batch_fwd(pose_adj.contiguous().float(), kinv.contiguous().float(),
                                                      self.weights_lens.detach().contiguous(), [cam], [0, npix], self.img_h, self.img_w,
                                                      pix=self._all_pix)
        return rays_d, rays_o

    # ------------------------------------------------------------------ forward (:58-122)
    def forward(self, *args):
        if self.sys_param["mode"] == 0:
            return self._forward_train(*args)
        return self._forward_demo(args[0] if len(args) == 1 else args)

    def _forward_train(self, data, epoch, epoch_type, cur_ratio):
        cam = int(data[1].reshape(-1)[0])          # read the camera id on the host side, before the H2D copy
        images = data[0] if isinstance(data[0], DeviceImageSet) else None      # device-resident uint8 images (row f3)
        # (the image index stays on the host: it is only ever used as a python index)
        gt_rgbs, _, intr_wpts, intr_pts, extr_wpts, extr_pts = [
            t if isinstance(t, DeviceImageSet) or i == 1 else t.to(self.device) for i, t in enumerate(data)]
        loss_dict = {}
        emb = self.nerf.emmbedding_xyz
        if epoch_type == "CAM_PARAM_EPOCH":         # (always one camera, whatever cams_per_step)
            emb.barf_mode = False
            self.intr_adj, self.pose_adj, self.calib_pose_adj = self.add_weights2param(True, True, True, intr_wpts, extr_wpts)
            loss_dict["intr"] = [self._reproject(intr_wpts, self.intr_adj, self.calib_pose_adj, 0), intr_pts]
            loss_dict["extr"] = [self._reproject(extr_wpts, self.intr_adj, self.pose_adj, 1), extr_pts]
            self.opt_idx = 0
        else:
            K = self.cams_per_step
            cams = [cam] if K == 1 else [int(c) for c in data[1].reshape(-1).tolist()]
            if len(cams) != K:
                raise ValueError(f"cams_per_step = {K}: data[1] must hold exactly {K} camera ids, got {len(cams)}")
            self._forward_train_nerf(cams, images, gt_rgbs, intr_wpts, intr_pts, epoch, epoch_type, cur_ratio, loss_dict)
        # validation rays of the same index, every step, as the reference (:97-99)
        with torch.no_grad():
            rays_dv, rays_ov = self.get_rays(self.valid_pose, cam, self.intr_val_inv)
            rays_valid = [rays_dv, rays_ov, self.valid_rgbs[cam:cam + 1].detach()]
        intr_show = [self.intr_train.detach(), self.intr_adj.detach()]
        pose_show = [self.gt_pose.detach(), self.pose_adj.detach()]
        self.last_epoch_type = epoch_type
        return loss_dict, intr_show, pose_show, rays_valid

    def _forward_train_nerf(self, cams, images, gt_rgbs, intr_wpts, intr_pts, epoch, epoch_type, cur_ratio, loss_dict):
        """The NeRF-stage step over K = len(cams) cameras (duplicates allowed): the batch is K segments of consecutive rays
        (`ops.ray_segments`), segment k of camera cams[k]; the renderer and the loss see an ordinary [batch] ray set.  K = 1 is the
        one-segment table.  Where the rays come from is all that differs:
          K = 1, pinhole: the pixels of `sample_pixels` (or the error draw), RaygenFn on that camera's matrices, the ground truth
                  gathered afterwards (the default step: a launch each);
          otherwise: ONE launch (RayBatchFn: pixels, rays, ground truth) that reads `pose_adj [C,3,4]` / `intr_inv_adj [C,3,3]` (and
                  `weights_lens [C,2]`) of all cameras as CameraFn left them.  K = 1 injects the same draw as above; K > 1 injects the
                  `sample_pixels_multi` hook's ids, else the error draw, else every segment draws in the kernel."""
        K, npix = len(cams), self.img_h * self.img_w
        if intr_wpts.shape[0] == K:        # a loader that batches K items stacks the (identical) calibration tensors K times
            intr_wpts, intr_pts = intr_wpts[:1], intr_pts[:1]
        joint = epoch_type == "GLOBAL_OPTIM_EPOCH"
        self.nerf.emmbedding_xyz.barf_mode = joint                  # :74 / :86
        self.intr_adj, self.pose_adj, self.calib_pose_adj = self.add_weights2param(True, joint, True, intr_wpts, None)
        loss_dict["intr"] = [self._reproject(intr_wpts, self.intr_adj, self.calib_pose_adj, 0), intr_pts]
        error, radial = self.pixel_sampler == "error", self.lens_model == "radial"
        if self.mask_weight > 0.0:
            if not self.weights_pose.is_cuda:
                raise ops._lib.McnerfError(f"mask_weight = {self.mask_weight}: mask supervision runs on the GPU only, the model is on {self.weights_pose.device}")
            if images is None or images.images.shape[2] != 4:
                raise ValueError(f"mask_weight = {self.mask_weight} needs a device-resident RGBA image set (DeviceImageSet, 4 channels), got "
                                 + ("a host float image stack" if images is None else f"{images.images.shape[2]}-channel images"))
        if self.dist_weight > 0.0 and not self.weights_pose.is_cuda:
            raise ops._lib.McnerfError(f"dist_weight = {self.dist_weight}: the distortion term runs on the GPU only, the model is on {self.weights_pose.device}")
        if self.depth_weight > 0.0:
            if not self.weights_pose.is_cuda:
                raise ops._lib.McnerfError(f"depth_weight = {self.depth_weight}: depth supervision runs on the GPU only, the model is on {self.weights_pose.device}")
            if images is None or getattr(images, "depth", None) is None:
                raise ValueError(f"depth_weight = {self.depth_weight} needs a device-resident image set with depth (DeviceImageSet(..., depth=...)), got "
                                 + ("a host float image stack" if images is None else "an image set without depth"))
        seg_start = ops.ray_segments(self.batch, K)
        if K == 1:      # pixel subset first (same device randperm as :329), rays only for those pixels
            pix = self._draw_error_pixels(cams, seg_start) if error else self.sample_pixels(npix)
            seg_start = [0, int(pix.shape[0])]                      # (`sample_pixels` returns min(batch, npix) ids)
        else:
            pix = self.sample_pixels_multi(npix, seg_start)
            if pix is None and error:                               # (an injected draw still wins)
                pix = self._draw_error_pixels(cams, seg_start)
        if K == 1 and not radial:
            cam = cams[0]
            kinv = self.intr_inv_adj[cam] if self.intr_inv_adj is not None else self.inverse_intrinsic(self.intr_adj[cam:cam + 1])[0]
            rays_d, rays_o = RaygenFn.apply(self.pose_adj[cam], kinv, pix, self.img_w)
            gt = None
        else:
            kinv_all = self.intr_inv_adj if self.intr_inv_adj is not None else self.inverse_intrinsic(self.intr_adj)
            pix, rays_d, rays_o, gt = RayBatchFn.apply(self.pose_adj, kinv_all, cams, seg_start, self.img_h, self.img_w,
                                                       images.images if images is not None else None, pix, None,
                                                       self.weights_lens if radial else None)
        rgbs_c, rgbs_f = self.nerf(rays_d, rays_o, epoch, cur_ratio if joint else 1)
        if gt is None and K == 1:
            gt = images.gather(cams[0], pix) if images is not None else gt_rgbs.reshape(-1, 3)[pix]
        elif gt is None:                   # host float stack [K,H,W,3] / [K,H*W,3]: item k is the image of segment k
            if self._seg_index is None:
                self._seg_index = ops.ray_segment_index(self.batch, K, pix.device)
            gt = gt_rgbs.reshape(K, -1, 3)[self._seg_index, pix]
        loss_dict["rgb"] = [rgbs_c, rgbs_f, gt]
        if self.color_calib == "affine":
            loss_dict["color"] = [self.weights_color, cams, seg_start]
        if self.mask_weight > 0.0:
            loss_dict["mask"] = [*self.nerf.last_front_weight, ops.gather_alpha(images.images, cams, seg_start, pix.contiguous())]
        if self.dist_weight > 0.0:
            loss_dict["dist"] = [*self.nerf.last_distortion]
        if self.depth_weight > 0.0:
            loss_dict["depth"] = [*self.nerf.last_expected_depth, ops.gather_depth(images.depth, cams, seg_start, pix.contiguous())]
        self.opt_idx = 1 if joint else 2
        if K > 1 or error:
            self.last_step_segments, self.last_step_pix = (cams, seg_start), pix
        if error:
            self._update_error_map(cams, seg_start, pix, rgbs_f, gt)

    def sample_pixels_multi(self, npix, seg_start):
        """Hook of the multi-camera step: pixel ids [batch] to inject (segment k's at [seg_start[k], seg_start[k+1])), or None (the
        default) = every segment draws its own subset without replacement on the device, inside the fused kernel; parity tests
        replace this method."""
        return None

    def sample_pixels(self, npix):
        """The step's pixel subset, randperm(npix)[:batch] of the reference (:329): on the GPU one kernel
        (``ops.sample_perm``, keyed from torch's device generator); parity tests replace this method to inject the
        reference's draw."""
        if self.weights_pose.is_cuda:
            return ops.sample_perm(npix, min(self.batch, npix), self.weights_pose.device)
        return torch.randperm(npix, device=self.device)[: self.batch]

    @torch.no_grad()
    def render_image_device(self, img_id, as_camera=None):
        """The demo render of one test camera (:106-122) with the result left on the device.  `as_camera` = c (color_calib =
        "affine"): the colours as training camera c is modelled to observe them, gain[c] * rgb + bias[c]; None (the default): the
        canonical, uncorrected scene."""
        rays_d, rays_o = self.get_rays(self.test_pose, img_id, self.intr_test_inv)
        rgb, depth, opacity = self.nerf.render_chunked(rays_d, rays_o, self.nerf.nerf_coarse, self.nerf.nerf_fine, chunk=self.batch)
        if as_camera is not None:
            gain, bias = self.color_correction()
            c = _int_key({"as_camera": as_camera}, "as_camera", None, 0, self.train_numb - 1)
            rgb = gain[c] * rgb + bias[c]
        return rgb, depth, opacity

    @torch.no_grad()
    def _forward_demo(self, img_id):
        rgb, depth, opacity = self.render_image_device(img_id)
        return rgb.cpu(), depth.cpu(), opacity.cpu()

    # ------------------------------------------------------------------ rays (:124-145, 327-345)
    def get_rays(self, pose, img_id, intr_inv):
        """All H*W rays of camera ``img_id`` (row-major pixel centres), differentiable wrt the
        selected pose and inverse intrinsics."""
        cam = int(torch.as_tensor(img_id).reshape(-1)[0])
        if getattr(self, "_all_pix", None) is None:
            self._all_pix = torch.arange(self.img_h * self.img_w, device=self.device)
        return RaygenFn.apply(pose[cam].to(self.device), intr_inv[cam].to(self.device), self._all_pix, self.img_w)

    def generate_rand_rays(self, rays_d, rays_o, rand=True):
        if rand:
            idx = torch.randperm(rays_d.shape[0], device=rays_d.device)[: self.batch]
        else:
            start = (self.count_rays * self.batch) % rays_d.shape[0]
            idx = torch.arange(start, min(start + self.batch, rays_d.shape[0]), device=rays_d.device)
        self.count_rays += 1
        return rays_d[idx], rays_o[idx], idx

    # ------------------------------------------------------------------ camera parametrisation (:155-210, 269-316)
    # On the GPU all six parameter tensors go through ONE fused kernel each way (CameraFn, csrc/camera.hip;
    # SURVEY.md 8f row f1).  The per-piece torch methods below restate the same maths; they serve host tensors
    # (the CPU plumbing tests of the camera-only stage) and API compatibility.
    def add_weights2param(self, intr=True, extr=True, calib_extr=False, intr_wpts=None, extr_wpts=None):
        """K, pose, calib pose of all cameras.  On the GPU the fused kernel also projects the calibration points
        (`intr_wpts` through (K, calib pose), `extr_wpts` through (K, pose); [1,C,P,3] as the loader delivers them, :374-386):
        the pixels are kept in `self._reproj` for `_reproject`, so the whole camera preamble is one launch each way."""
        self.intr_inv_adj = None
        self._reproj = [None, None]
        if self.weights_pose.is_cuda:
            det = lambda t, on: t if on else t.detach()
            pts = [None if t is None else t.reshape(-1, t.shape[-2], 3) for t in (intr_wpts, extr_wpts)]
            K, Kinv, pose, calib, pi, pe = CameraFn.apply(det(self.weights_pose, extr), det(self.weights_pose_intr, calib_extr),
                                                          det(self.weights_fx, intr), det(self.weights_fy, intr),
                                                          det(self.weights_ux, intr), det(self.weights_uy, intr),
                                                          self.img_h, self.img_w, pts[0], pts[1])
            self.intr_inv_adj = Kinv
            self._reproj = [None if pi is None else pi.reshape(intr_wpts.shape[:-1] + (2,)),
                            None if pe is None else pe.reshape(extr_wpts.shape[:-1] + (2,))]
            return K, pose, calib
        return (self.add_weights2intr(self.img_h, self.img_w, adj=intr), self.add_weights2pose(adj=extr),
                self.add_weights2calib_pose(adj=calib_extr))

    def add_weights2intr(self, img_h, img_w, adj=True):
        w = [self.weights_fx, self.weights_fy, self.weights_ux, self.weights_uy]
        if not adj:
            w = [t.detach() for t in w]
        C = self.train_numb
        K = torch.zeros(C, 3, 3, device=self.device)
        # note: the reference scales fy by the image WIDTH as well (:172-173)
        K[:, 0, 0] = torch.abs(float(img_w) * w[0])
        K[:, 1, 1] = torch.abs(float(img_w) * w[1])
        K[:, 0, 2] = torch.abs(float(img_w) / 2 * w[2])
        K[:, 1, 2] = torch.abs(float(img_h) / 2 * w[3])
        K[:, 2, 2] = 1.0
        return K

    def add_weights2pose(self, adj=True):
        return self.se3_to_SE3(self.weights_pose if adj else self.weights_pose.detach())

    def add_weights2calib_pose(self, adj=True):
        return self.se3_to_SE3(self.weights_pose_intr if adj else self.weights_pose_intr.detach())

    def inverse_intrinsic(self, intr_mats):
        return torch.linalg.inv(intr_mats)

    @staticmethod
    def _series(theta, first_factor, nth=10):
        """sum_i (-1)^i theta^(2i) / denom_i with denom_0 = first_factor and
        denom_i = denom_{i-1} * (2i+a)(2i+a+1): the Taylor series A, B, C of :291-316."""
        a = {1.0: 0, 2.0: 1, 6.0: 2}[first_factor]
        ans = torch.zeros_like(theta)
        denom = 1.0
        for i in range(nth + 1):
            if a == 0:
                if i > 0:
                    denom *= (2 * i) * (2 * i + 1)
            else:
                denom *= (2 * i + a) * (2 * i + a + 1)
            ans = ans + (-1) ** i * theta ** (2 * i) / denom
        return ans

    def se3_to_SE3(self, wu):
        w, u = wu[..., :3], wu[..., 3:]
        O = torch.zeros_like(w[..., 0])
        wx = torch.stack([torch.stack([O, -w[..., 2], w[..., 1]], -1),
                          torch.stack([w[..., 2], O, -w[..., 0]], -1),
                          torch.stack([-w[..., 1], w[..., 0], O], -1)], -2)
        theta = w.norm(dim=-1)[..., None, None]
        I = torch.eye(3, device=wu.device)
        A, B, Cc = self._series(theta, 1.0), self._series(theta, 2.0), self._series(theta, 6.0)
        R = I + A * wx + B * wx @ wx
        V = I + B * wx + Cc * wx @ wx
        return torch.cat([R, V @ u[..., None]], dim=-1)

    # ------------------------------------------------------------------ reprojection branch (:147-152, 236-267)
    def _reproject(self, tag_wpts, intr_adj, pose_adj, which):
        """The pixels the fused camera kernel already produced (GPU), else the tensor-op restatement."""
        got = getattr(self, "_reproj", [None, None])[which]
        pix = got if got is not None else self.get_reproject_pixels(tag_wpts, intr_adj, pose_adj)
        if self.lens_model == "radial":      # the tags of a distorted camera are observed at distorted pixels (closed form, eager)
            pix = distort_pixels(pix, intr_adj, self.weights_lens)
        return pix

    def get_reproject_pixels(self, tag_wpts, intr_adj, pose_adj):
        """Projects calibration points [B,C,P,3] through [R|t] and K -> pixel coords [B,C,P,2]."""
        ones = torch.ones_like(tag_wpts[..., :1])
        wh = torch.cat([tag_wpts, ones], dim=-1)                       # [B,C,P,4]
        cam = wh @ pose_adj.unsqueeze(0).transpose(-2, -1)             # [B,C,P,3]
        pix = cam @ intr_adj.unsqueeze(0).transpose(-2, -1)
        return pix[..., :2] / pix[..., 2:]

    # ------------------------------------------------------------------ reporting hooks used by main.py
    def show_estimate_param(self, intr_show, pose_show, epoch, epoch_type):
        intr_err = (intr_show[0] - intr_show[1]).abs()
        pose_err = (pose_show[0] - pose_show[1]).abs()
        logging.info("EPOCH {} |K err| fx {:.4f} fy {:.4f} ux {:.4f} uy {:.4f} | R {:.5f} T {:.5f}".format(
            epoch, float(intr_err[:, 0, 0].mean()), float(intr_err[:, 1, 1].mean()), float(intr_err[:, 0, 2].mean()),
            float(intr_err[:, 1, 2].mean()), float(pose_err[..., :3].mean()), float(pose_err[..., 3].mean())))

    def show_RT_est_results(self, epoch, epoch_type=None, mode="epoch", show_info=True):
        """Reference signature (:388); main.py:94 calls show_RT_est_results(epoch, epoch_type, mode='epoch').  The
        reference aligns the estimated poses to the ground truth and plots the camera frusta; here the alignment-free
        pose error is logged (plotting is outside the hot path)."""
        if show_info and hasattr(self, "pose_adj"):
            err = (self.gt_pose - self.pose_adj.detach()).abs()
            logging.info("EPOCH {} [{}] pose |R err| {:.5f} |t err| {:.5f}".format(epoch, epoch_type, float(err[..., :3].mean()),
                                                                                   float(err[..., 3].mean())))
