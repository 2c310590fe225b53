"""Autograd glue between the reference-shaped Python API and the HIP kernels.

The render pipeline (reference: model/mc_nerf.py:598-680) is two PASSES, each a net evaluated on a sample set and composited.  A
``SamplePass`` record describes one: the net, the depths (the shared grid plus per-ray jitter, or per-ray rows), the [N,S,4] output, an
optional (ray, sample) list over a prefilled output, the saved-operand set of a training call.  ``run_pass`` runs it (ops.mlp_fwd,
ops.composite_fwd), ``pass_backward`` differentiates it (composite bwd -> dX chain -> dW).  ``coarse_pass`` and ``fine_pass`` build the
two passes of a render; ``RenderTrainFn`` (ONE differentiable op for NeRF_Model.render_rays_train, with that hand-written backward
instead of autograd through ~900 ATen ops), ``render_test`` and NeRF_Model._inference run what they return.  ``RaygenFn`` is the
same kind of op for MC_Model.get_rays on selected pixels of one camera, ``RayBatchFn`` for a batch that spans cameras and for the
radial lens model (its ``lens`` input; None = pinhole), ``CameraFn`` for the camera parametrisation.

What a sampler setting changes in its pass:
  fine_sampler "threshold" (the reference): the list ops.select_fine compacts from the coarse selection weights, over the
      (sigma_default, 1, 1, 1) prefill of the fine grid; training caps it at 128 per ray.
  fine_sampler "pdf": dense per-ray depth rows, ops.sample_pdf's sorted [coarse + n_importance inverse-CDF] depths (a constant of
      the pass: no gradient through the sampler); the rows hold the jitter.
  coarse_sampler "voxel": the list ops.voxel_select reads off the owner's sigma grid, over the prefill.  Train calls keep the grid
      current from their evaluated samples (ops.voxel_update) and run dense in the warm-up; rendering only queries.
  ray_bounds_miss "skip" ("aabb" mode): every pass is a listed one, its list built behind the per-ray hit flag (ops.list_rays, or
      `hit=` of ops.select_fine / ops.voxel_select): no sample of a ray that misses the box reaches a net, its rows stay the prefill.
  ray_bounds_fit "voxel" ("aabb" mode): the box of `bounds_rows` is the owner's device tensor, fitted to the sigma grid (ops.voxel_box);
      downstream of the rows and flags nothing changes.
  ray_bounds "aabb": both passes take per-ray rows (`bounds_rows`: ops.ray_depths on the scene box; the rows hold the jitter) where
      they took the shared grid plus jitter: the voxel list and update, the pdf sampler and the threshold fine pass, which is then a
      listed pass on rows [N,Sf].  The rows are constants of the backward.

Every random draw of the reference (jitter, the three N(0,1) tensors of sigma2weights, the cap permutation; in "pdf" mode the
sampler's U(0,1) draws) is an explicit tensor argument: drawn from torch's device RNG by the caller, or passed in by the parity tests.
"""
from __future__ import annotations

from collections import namedtuple
from contextlib import AbstractContextManager
from dataclasses import dataclass
from typing import Optional

import torch

from .. import ops


@dataclass
class RenderSettings:
    """The renderer constants the kernels need (reference: model/mc_nerf.py:548-571)."""
    samples_c: int
    scale: int
    weight_thresh: float
    sigma_default: float
    white_back: bool
    max_fine_per_ray: int = 128      # model/mc_nerf.py:630
    # "f32": exact-fp32 MFMA; "f16x3": split-f16 MFMA (fp32-grade: the 1e-4 parity modes); "f16" / "bf16": single-pass
    # 16-bit MFMA with 2-byte workspaces (throughput modes, accuracy of the operand rounding: csrc/mcnerf_16.h)
    precision: str = "f32"
    # "threshold": the reference's weight-threshold refinement (model/mc_nerf.py:613-632); "pdf": inverse-CDF hierarchical
    # sampling of n_importance depths per ray, the fine net evaluated on Sc + n_importance sorted depths per ray
    fine_sampler: str = "threshold"
    n_importance: int = 128
    # "dense": the coarse net on the whole [N,Sc] grid (the reference); "voxel": on the (ray, sample) pairs whose cell of the owner's
    # sigma grid holds a raw sigma > voxel_thresh (ops.voxel_select), the grid kept current by train calls (ops.voxel_update, rate
    # voxel_beta); train calls with cur_epoch < voxel_warmup_epoch run the dense pass and only update the grid
    coarse_sampler: str = "dense"
    voxel_beta: float = 0.1
    voxel_thresh: float = 0.0
    voxel_warmup_epoch: int = 1
    # "global": every ray on linspace(near, far) (the reference); "aabb" (DESIGN.md 4k): every ray on its own rows of depths, the grids
    # mapped onto the part of [near, far] inside `box` = (xmin, ymin, zmin, xmax, ymax, zmax) (ops.ray_depths).  (Ahead of want_zexp: its place at the end of the field list is pinned.)
    ray_bounds: str = "global"
    box: Optional[tuple] = None
    # read in "aabb" mode only.  "sample": a ray that misses the box is sampled on [near, far] (today's launches and bits;
    # the hit library is not loaded); "skip": neither net evaluates a sample of it -- both passes are listed passes over the prefill, their
    # lists built behind the per-ray hit flag of ops.ray_depths
    ray_bounds_miss: str = "sample"
    # read in "aabb" mode only.  "fixed": the box is `box` (today's launches and bits; the fit library is not loaded);
    # "voxel" (needs coarse_sampler "voxel"): the box is fitted on the device to the cells of the sigma grid above voxel_thresh, padded by
    # ray_bounds_fit_margin cells and clamped to `box`, the OUTER box, which is also the box in force until the first fit; train calls
    # past the warm-up refit it every ray_bounds_fit_every calls (ops.voxel_box; NeRF_Model.refit_scene_box)
    ray_bounds_fit: str = "fixed"
    ray_bounds_fit_margin: int = 2
    ray_bounds_fit_every: int = 16
    # depth mode: each pass's expected depth on the rgb composite's own weights is one more differentiable output of
    # the train render.  The switch rides here, not on RenderCall (its field list is pinned); NeRF_Model sets it from "depth_weight"
    want_zexp: bool = False

    @property
    def aabb(self) -> bool:
        return self.ray_bounds == "aabb"

    @property
    def skip_misses(self) -> bool:
        return self.aabb and self.ray_bounds_miss == "skip"

    @property
    def fit_box(self) -> bool:
        return self.aabb and self.ray_bounds_fit == "voxel"

    @property
    def samples_f(self):
        return self.samples_c * self.scale

    @property
    def samples_pdf(self):
        """Depths per ray of the fine pass in "pdf" mode: the coarse ones and the importance samples."""
        return self.samples_c + self.n_importance

    @property
    def pdf(self) -> bool:
        return self.fine_sampler == "pdf"

    @property
    def voxel(self) -> bool:
        return self.coarse_sampler == "voxel"

    def fine_rows(self, n_rays: int, train: bool) -> int:
        """Row capacity of the fine pass; the cap of model/mc_nerf.py:630-632 (128 per ray) applies in training only."""
        if self.pdf:
            return n_rays * self.samples_pdf
        return n_rays * (min(self.samples_f, self.max_fine_per_ray) if train else self.samples_f)


class WorkspacePool:
    """The MLP kernels' saved-operand and gradient workspaces (up to ~46 GB per step at 32768 rays in the split-f16 mode), sized
    ONCE per (net, row capacity, precision) and handed from step to step instead of going through the allocator every forward /
    backward: RenderTrainFn.forward takes a set, .backward gives it back after the weight-gradient kernel has been enqueued
    (stream order makes the re-use safe: the next forward's stores are behind that kernel).  A forward whose backward never
    runs simply keeps its set (garbage-collected with the graph); a second forward before the first backward gets a fresh one.
    `NeRF_Model.reserve_workspaces(n_rays)` fills the pool before the first step (multi-GPU: no first-step allocation in any
    rank between two barriers)."""
    MAX_KEYS = 6

    def __init__(self):
        self.free = {}

    def _key(self, kind, net, capacity, device, precision):
        return (kind, net.triple, int(capacity), str(device), precision)

    def _take(self, key, make):
        lst = self.free.get(key)
        return lst.pop() if lst else make()

    def _give(self, key, ws):
        if key not in self.free and len(self.free) >= self.MAX_KEYS:
            self.free.pop(next(iter(self.free)))            # (a changing shape -- test paths -- must not pin memory for ever)
        self.free.setdefault(key, []).append(ws)

    def take_save(self, net, capacity, device, precision):
        return self._take(self._key("save", net, max(int(capacity), 1), device, precision), lambda: ops.alloc_save(net, capacity, device, precision=precision))

    def give_save(self, net, save, precision):
        self._give(self._key("save", net, save.capacity, save.act.device, precision), save)

    def take_grad(self, net, save, precision):
        return self._take(self._key("grad", net, save.capacity, save.act.device, precision), lambda: ops.alloc_grad_ws(net, save, precision))

    def give_grad(self, net, save, precision, ws):
        self._give(self._key("grad", net, save.capacity, save.act.device, precision), ws)


class WorkspaceLease(AbstractContextManager):
    """The sets ONE forward or backward holds from the pool.  When an exception leaves its `with` block (a range overflow raised by a
    kernel, out of memory in a take) everything still held goes back: a retried step must find the pool as it was, not one set short.
    Otherwise the sets stay held: the forward leaves its lease with ctx, the backward gives each set back (`give`) once everything that
    reads it is enqueued.  `held` = (set, the pool's method that takes it back, its arguments) in the order taken; nothing in it refers
    to the lease: a forward whose backward never runs frees its tens of GB with the graph, by reference count, not by the cycle collector."""

    def __init__(self, pool: WorkspacePool, precision):
        self.pool, self.precision, self.held = pool, precision, []

    def take_save(self, net, capacity, device):
        save = self.pool.take_save(net, capacity, device, self.precision)
        self.held.append((save, self.pool.give_save, (net, save, self.precision)))
        return save

    def take_grad(self, net, save):
        ws = self.pool.take_grad(net, save, self.precision)
        self.held.append((ws, self.pool.give_grad, (net, save, self.precision, ws)))
        return ws

    def give(self, ws):
        _, back, args = self.held.pop(next(i for i, entry in enumerate(self.held) if entry[0] is ws))
        back(*args)

    def __exit__(self, exc_type, exc, tb):
        while exc_type is not None and self.held:
            self.give(self.held[-1][0])                     # (the set taken last first)


def _pool(owner) -> WorkspacePool:
    if getattr(owner, "ws_pool", None) is None:
        owner.ws_pool = WorkspacePool()
    return owner.ws_pool


# What both passes of a render share: origins and directions [N,3] (contiguous) and the BARF weights of the encoding.
Rays = namedtuple("Rays", "o d barf_w")


@dataclass
class SamplePass:
    """One net evaluated on one sample set and composited.  Holds references only.  Depths: the shared `zgrid` [S] plus `jitter` [N]
    (None: no jitter), or per-ray `z_rows` [N,S] (zgrid and jitter None).  `idx` / `count` / `max_rows`: the (ray, sample) list the
    net runs on over the prefilled `out`, None / None / 0 = every sample.  `save`: the saved-operand set of a training call."""
    model: object
    flat: torch.Tensor
    packed: torch.Tensor
    zgrid: Optional[torch.Tensor]
    jitter: Optional[torch.Tensor]
    z_rows: Optional[torch.Tensor]
    eps: torch.Tensor
    out: torch.Tensor
    idx: Optional[torch.Tensor] = None
    count: Optional[torch.Tensor] = None
    max_rows: int = 0
    save: Optional[ops.MlpSave] = None
    moments: Optional[torch.Tensor] = None      # distortion mode: ops.distortion_fwd's per-ray sums, for the backward

    TENSORS = ("flat", "packed", "zgrid", "jitter", "z_rows", "eps", "out", "idx", "count", "moments")

    @property
    def rows(self) -> int:
        """Rows the net is evaluated on at the most: the saved-operand set's capacity, and the row count the dW kernel takes."""
        return self.max_rows if self.idx is not None else self.out.shape[0] * self.out.shape[1]

    def tensors(self):
        """For ctx.save_for_backward; `restored` takes them off the front of an iterator over ctx.saved_tensors."""
        return tuple(getattr(self, name) for name in self.TENSORS)

    @classmethod
    def restored(cls, model, saved, max_rows, save):
        return cls(model, **{name: next(saved) for name in cls.TENSORS}, max_rows=max_rows, save=save)


def run_pass(p: SamplePass, st: RenderSettings, rays: Rays, lease: Optional[WorkspaceLease] = None, eps_sel=None, want_depth=False):
    """The net on the pass's samples, then the composite -> ops.composite_fwd's (rgb, depth, opacity, w_sel, wmax).  With a `lease`
    the operands of the backward are saved, in a set taken through it."""
    net = p.model.net
    if lease is not None:
        p.save = lease.take_save(net, p.rows, rays.d.device)
    ops.mlp_fwd(net, p.flat, p.packed, rays.o, rays.d, p.zgrid, p.jitter, rays.barf_w, p.out,
                idx=p.idx, count=p.count, max_rows=p.max_rows, save=p.save, precision=st.precision, z_rows=p.z_rows)
    return ops.composite_fwd(p.out, rays.d, p.zgrid, p.jitter, p.eps, eps_sel, st.white_back, want_depth=want_depth, z_rows=p.z_rows)


def front_weight(p: SamplePass):
    """fg [N] of a pass that `run_pass` has composited (ops.front_weight: the rgb composite's weights in front of the far-plane sample)."""
    return ops.front_weight(p.out, p.zgrid, p.jitter, p.eps, z_rows=p.z_rows)


def distortion(p: SamplePass, span):
    """dist [N] of a pass that `run_pass` has composited (ops.distortion_fwd on the depth range `span` = (near, far)); the per-ray sums
    its backward needs stay with the pass."""
    dist, p.moments = ops.distortion_fwd(p.out, p.zgrid, p.jitter, p.eps, *span, z_rows=p.z_rows)
    return dist


def expected_depth(p: SamplePass):
    """zexp [N] of a pass that `run_pass` has composited (ops.expected_depth: sum w z on the rgb composite's weights, the far-plane
    sample included)."""
    return ops.expected_depth(p.out, p.zgrid, p.jitter, p.eps, z_rows=p.z_rows)


def pass_backward(p: SamplePass, st: RenderSettings, rays: Rays, d_rgb, grads, d_o, d_d, lease: WorkspaceLease, d_fg=None, d_dist=None,
                  span=None, d_zexp=None):
    """The pass's composite backward, dX chain (into d_o / d_d [N,3] when given) and weight gradients (into `grads`); nothing when
    `d_rgb`, `d_fg`, `d_dist` and `d_zexp` are None.  Either way the pass's saved-operand set goes back to the pool.  `d_fg` [N] (mask mode): the
    gradient on the pass's front weight; the composite backward is then the extension library's, which takes both (d_rgb None: zeros).
    `d_dist` [N] (distortion mode, with `span` = (near, far)): the gradient on the pass's distortion term; the composite backward is
    then the regulariser library's, which takes all three.  `d_zexp` [N] (depth mode): the gradient on the pass's expected depth; the
    composite backward is then the geometry library's, which takes whatever of the other gradients is there."""
    net = p.model.net
    if d_rgb is not None or d_fg is not None or d_dist is not None or d_zexp is not None:
        if d_zexp is not None:
            d_rgb = torch.zeros(p.out.shape[0], 3, dtype=torch.float32, device=p.out.device) if d_rgb is None else d_rgb.contiguous()
            d_out, gmax = ops.composite_bwd_z(p.out, p.zgrid, p.jitter, p.eps, d_rgb, None if d_fg is None else d_fg.contiguous(),
                                              None if d_dist is None else d_dist.contiguous(), p.moments, d_zexp.contiguous(), *span,
                                              st.white_back, want_gmax=True, z_rows=p.z_rows)
        elif d_dist is not None:
            d_rgb = torch.zeros(p.out.shape[0], 3, dtype=torch.float32, device=p.out.device) if d_rgb is None else d_rgb.contiguous()
            d_out, gmax = ops.composite_bwd_w(p.out, p.zgrid, p.jitter, p.eps, d_rgb, None if d_fg is None else d_fg.contiguous(),
                                              d_dist.contiguous(), p.moments, *span, st.white_back, want_gmax=True, z_rows=p.z_rows)
        elif d_fg is not None:
            d_rgb = torch.zeros(p.out.shape[0], 3, dtype=torch.float32, device=p.out.device) if d_rgb is None else d_rgb.contiguous()
            d_out, gmax = ops.composite_bwd_front(p.out, p.zgrid, p.jitter, p.eps, d_rgb, d_fg.contiguous(), st.white_back,
                                                  want_gmax=True, z_rows=p.z_rows)
        else:
            d_out, gmax = ops.composite_bwd(p.out, p.zgrid, p.jitter, p.eps, d_rgb.contiguous(), st.white_back, want_gmax=True, z_rows=p.z_rows)
        dy, dsh = ws = lease.take_grad(net, p.save)
        ops.mlp_bwd(net, p.flat, p.packed, rays.o, rays.d, p.zgrid, p.jitter, rays.barf_w, p.out, d_out, p.save, dy, dsh,
                    d_o, d_d, idx=p.idx, count=p.count, max_rows=p.max_rows, precision=st.precision, gmax=gmax, z_rows=p.z_rows)
        ops.mlp_dw(net, p.save, dy, dsh, grads, p.rows, count=p.count, precision=st.precision, gmax=gmax)
        lease.give(ws)
    lease.give(p.save)


def select_and_cap(st: RenderSettings, w_sel, wmax, n_rays, cap_perm, train: bool, hit=None):
    """Device-side selection; applies the random cap in training.  Returns idx, count, out_f, max_rows.  `hit` [N] (skipping the rays
    that miss the box): only rays with hit[n] != 0 are selected from; the cap then acts on that list, with the same row capacities.
    No host synchronisation: the cap's random subset is drawn on the device (ops.cap_random) with a seed word taken
    from torch's device generator.  Only a caller-supplied permutation (`cap_perm`, the parity-test input that replays
    the reference's CPU randperm, :631) goes through the host: its length IS the host-side count."""
    idx, count, out_f = ops.select_fine(w_sel, wmax, st.weight_thresh, st.scale, st.sigma_default, hit=hit)
    max_rows, keep = st.fine_rows(n_rays, train=False), st.fine_rows(n_rays, train=True)
    if train and keep < max_rows:
        if cap_perm is not None:
            k = int(count.item())                  # (test path only)
            if k > keep:
                perm = cap_perm[:keep].to(device=idx.device, dtype=torch.int64).contiguous()
                idx, count = ops.cap_gather(idx, perm, keep)
                max_rows = keep
            else:
                max_rows = min(max_rows, max(k, 1))
        else:
            idx, count = ops.cap_random(idx, count, max_rows, keep, ops.seed_word(idx.device))
            max_rows = keep
    return idx, count, out_f, max_rows


def bounds_rows(owner, rays: Rays, jitter):
    """(z_c [N,Sc], z_f [N,Sf] | None, hit [N] int32 | None) of a render in "aabb" mode -- the model's own grids mapped onto every ray's
    part of [near, far] inside the box, jitter included (ops.ray_depths; z_f in "threshold" mode only: the pdf sampler draws its own
    fine depths), and with `ray_bounds_miss` = "skip" the flag of the rays the box clips, from the same launch -- and None in "global"
    mode, where nothing is allocated.  The (lo, hi) of every ray stays with the owner in `last_ray_span`, the flags in `last_ray_hit`.
    This is the one place that hands the box to the kernel: `settings.box`, or with `ray_bounds_fit` = "voxel" the owner's fitted box, a
    device tensor that the kernel reads itself (it stays with the owner in `last_scene_box`)."""
    st: RenderSettings = owner.settings
    if not st.aabb:
        return None
    if not rays.d.is_cuda:
        raise ops._lib.McnerfError(f"ray_bounds = 'aabb': the per-ray depths are a HIP kernel, got rays on {rays.d.device} (no CPU fallback)")
    box = owner.last_scene_box = owner.scene_box if st.fit_box else None
    z_c, z_f, owner.last_ray_span, *hit = ops.ray_depths(rays.o, rays.d, st.box if box is None else box, float(owner.near), float(owner.far), jitter, owner.z_vals_c,
                                                         None if st.pdf else owner.z_vals_f, want_hit=st.skip_misses)
    owner.last_ray_hit = hit[0] if hit else None
    return z_c, z_f, owner.last_ray_hit


def coarse_pass(owner, model, flat, packed, rays: Rays, jitter, eps, prune: bool, rows=None) -> SamplePass:
    """The coarse pass: the dense [N,Sc] grid, or (`prune`, read in "voxel" mode only: a train call past the warm-up, or rendering)
    the sigma grid's list over the default prefill.  `rows` (`bounds_rows`; "aabb" mode): the depths are its coarse rows.  With its
    hit flags the pass is always a listed one: the grid's list behind the flag, or every sample of the rays that hit (ops.list_rays)."""
    st: RenderSettings = owner.settings
    N = rays.d.shape[0]
    grid = owner.voxel_grid() if st.voxel else None
    zgrid, jitter, z_rows = (owner.z_vals_c, jitter, None) if rows is None else (None, None, rows[0])
    hit = None if rows is None else rows[2]
    idx = count = None
    if grid is not None and prune:
        idx, count, out = ops.voxel_select(grid, st.voxel_thresh, rays.o, rays.d, zgrid, jitter, st.sigma_default, z_rows=z_rows, hit=hit)
    elif hit is not None:
        idx, count, out = ops.list_rays(hit, st.samples_c, st.sigma_default)
    else:
        out = torch.empty(N, st.samples_c, 4, dtype=torch.float32, device=rays.d.device)
    owner.last_coarse_selection = None if idx is None else (idx, count)
    return SamplePass(model, flat, packed, zgrid, jitter, z_rows, eps, out, idx, count, N * st.samples_c if idx is not None else 0)


def fine_pass(owner, model, flat, packed, rays: Rays, jitter, w_sel, wmax, eps, u, cap_perm, train: bool, rows=None) -> SamplePass:
    """The fine pass from the coarse composite's selection weights: the selected (ray, sample) list over the default prefill (no host
    sync), or in "pdf" mode dense rows of inverse-CDF depths drawn with `u`.  `rows` (`bounds_rows`; "aabb" mode): the sampler reads
    its coarse rows, the listed pass runs on its fine rows.  With its hit flags the selection is made behind them, and the "pdf" pass is
    a listed pass too, on the sampler's rows of the rays that hit."""
    st: RenderSettings = owner.settings
    hit = None if rows is None else rows[2]
    if st.pdf:
        z_all = ops.sample_pdf(w_sel, owner.z_vals_c, jitter, u) if rows is None else ops.sample_pdf(w_sel, None, None, u, z_rows=rows[0])
        if hit is not None:
            idx, count, out = ops.list_rays(hit, z_all.shape[1], st.sigma_default)
            p = SamplePass(model, flat, packed, None, None, z_all, eps, out, idx, count, z_all.shape[0] * z_all.shape[1])
        else:
            out = torch.empty(*z_all.shape, 4, dtype=torch.float32, device=rays.d.device)
            p = SamplePass(model, flat, packed, None, None, z_all, eps, out)
    else:
        idx, count, out, max_rows = select_and_cap(st, w_sel, wmax, rays.d.shape[0], cap_perm, train, hit)
        zgrid, jitter, z_rows = (owner.z_vals_f, jitter, None) if rows is None else (None, None, rows[1])
        p = SamplePass(model, flat, packed, zgrid, jitter, z_rows, eps, out, idx, count, max_rows)
    owner.last_selection, owner.last_z_all = None if p.idx is None else (p.idx, p.count), p.z_rows if st.pdf else None
    return p


def _packed(model, flat, st: RenderSettings, dev):
    return ops.pack_weights(model.net, flat, precision=st.precision, range_flags=model.range_flags(st.precision, dev))


# Everything non-differentiable of one RenderTrainFn call.  `prune` (read in "voxel" mode only): True = the coarse net runs on the
# grid's (ray, sample) list, False = the warm-up's dense pass; either way the grid is then updated from the evaluated samples.
# `want_fg` (mask mode): each pass's front weight is one more differentiable output.  `want_dist` (distortion mode,
# DESIGN.md 4i): so is each pass's distortion term.
RenderCall = namedtuple("RenderCall", "owner model_c model_f step_r only_coarse jitter eps_c eps_sel u eps_f cap_perm prune want_dist want_fg",
                        defaults=(False, False))


class RenderTrainFn(torch.autograd.Function):
    """rgb_c, rgb_f, depth_c, fg_c, fg_f, dist_c, dist_f, zexp_c, zexp_f = f(rays_d, rays_o, call, *coarse_params, *fine_params); `call` (RenderCall)
    holds the explicit draws.  fg_c / fg_f [N]: the passes' front weights with `call.want_fg`, else None (and nothing of the extension
    library runs).  dist_c / dist_f [N]: the passes' distortion terms with `call.want_dist`, else None (and nothing of the
    regulariser library runs).  zexp_c / zexp_f [N]: the passes' expected depths with `settings.want_zexp`, else None (and nothing of
    the geometry library runs); zexp_f is None after an only_coarse call."""

    @staticmethod
    def forward(ctx, rays_d, rays_o, call: RenderCall, *params):
        owner, st, dev = call.owner, call.owner.settings, rays_d.device
        need_grad = any(ctx.needs_input_grad)
        rays = Rays(d=rays_d.contiguous(), o=rays_o.contiguous(), barf_w=owner.emmbedding_xyz.barf_weights_on(call.step_r, dev, pad=10))
        jit = call.jitter.reshape(-1).contiguous()
        with WorkspaceLease(_pool(owner), st.precision) as lease:
            saving = lease if need_grad else None
            flat_c = call.model_c.flat_params()
            rows = bounds_rows(owner, rays, jit)
            coarse = coarse_pass(owner, call.model_c, flat_c, _packed(call.model_c, flat_c, st, dev), rays, jit, call.eps_c, call.prune, rows)
            rgb_c, depth_c, _, w_sel, wmax = run_pass(coarse, st, rays, saving, None if call.only_coarse else call.eps_sel,
                                                      want_depth=call.only_coarse)
            fg_c = front_weight(coarse) if call.want_fg else None
            span = (float(owner.near), float(owner.far))
            dist_c = distortion(coarse, span) if call.want_dist else None
            zexp_c = expected_depth(coarse) if st.want_zexp else None
            if st.voxel:
                ops.voxel_update(owner.voxel_grid(), st.voxel_beta, rays.o, rays.d, coarse.zgrid, coarse.jitter, coarse.out,
                                 coarse.idx, coarse.count, coarse.max_rows, z_rows=coarse.z_rows)
            passes, rgb_f, fg_f, dist_f, zexp_f = [coarse], None, None, None, None
            if not call.only_coarse:
                flat_f = call.model_f.flat_params()
                fine = fine_pass(owner, call.model_f, flat_f, _packed(call.model_f, flat_f, st, dev), rays, jit, w_sel, wmax,
                                 call.eps_f, call.u, call.cap_perm, train=True, rows=rows)
                rgb_f = run_pass(fine, st, rays, saving)[0]
                fg_f = front_weight(fine) if call.want_fg else None
                dist_f = distortion(fine, span) if call.want_dist else None
                zexp_f = expected_depth(fine) if st.want_zexp else None
                passes.append(fine)
        if need_grad:                                       # the lease, with the sets it holds, waits in ctx for the backward
            ctx.owner, ctx.model_f, ctx.lease = owner, call.model_f, lease          # (not `call`: it would keep every draw alive)
            ctx.stubs = [(p.model, p.max_rows, p.save) for p in passes]
            ctx.save_for_backward(*rays, *(t for p in passes for t in p.tensors()))
        if depth_c is not None:                             # (only_coarse; rgb_f is None then)
            ctx.mark_non_differentiable(depth_c)
        return rgb_c, rgb_f, depth_c, fg_c, fg_f, dist_c, dist_f, zexp_c, zexp_f

    @staticmethod
    def backward(ctx, d_rgb_c, d_rgb_f, _d_depth, d_fg_c=None, d_fg_f=None, d_dist_c=None, d_dist_f=None, d_zexp_c=None, d_zexp_f=None):
        if getattr(ctx, "workspaces_given_back", False):
            # retain_graph=True + a second backward: the saved-operand set went back to the pool after the first one and the next
            # forward may already have overwritten it -- refuse instead of returning gradients of clobbered operands
            raise ops._lib.McnerfError("RenderTrainFn.backward ran twice on one forward (retain_graph): its saved-operand workspaces were "
                                  "returned to the pool by the first backward; run the forward again")
        owner, st, model_f = ctx.owner, ctx.owner.settings, ctx.model_f
        saved = iter(ctx.saved_tensors)
        rays = Rays(next(saved), next(saved), next(saved))
        coarse, *fine = [SamplePass.restored(model, saved, max_rows, save) for model, max_rows, save in ctx.stubs]
        N, dev = rays.d.shape[0], rays.d.device
        span = (float(owner.near), float(owner.far))
        want_rays = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        d_od = torch.zeros(2, N, 3, dtype=torch.float32, device=dev) if want_rays else None      # (one fill for both)
        d_o, d_d = (d_od[0], d_od[1]) if want_rays else (None, None)
        # gradient buffers: slices of the step-level arena when a FlatGradSync provided one (so the whole
        # step's gradient is one contiguous all-reduce message), otherwise fresh zeroed buffers
        arena = getattr(owner, "grad_arena", None)
        n_c, n_f = coarse.flat.numel(), model_f.flat_params().numel()
        g_c = arena[:n_c] if arena is not None else torch.zeros_like(coarse.flat)
        g_f = None
        if arena is not None:
            owner.grad_arena_used = True
        # from here on the saved-operand sets leave this context, whatever happens: a second backward on a retained graph is refused
        lease, ctx.lease, ctx.stubs = ctx.lease, None, None
        ctx.workspaces_given_back = True
        with lease:
            for p in fine:                                  # (none after an only_coarse call)
                g_f = arena[n_c:n_c + n_f] if arena is not None else torch.zeros_like(p.flat)
                pass_backward(p, st, rays, d_rgb_f, g_f, d_o, d_d, lease, d_fg_f, d_dist_f, span, d_zexp_f)
            pass_backward(coarse, st, rays, d_rgb_c, g_c, d_o, d_d, lease, d_fg_c, d_dist_c, span, d_zexp_c)
        grads_c = coarse.model.grad_views(g_c)
        grads_f = model_f.grad_views(g_f) if g_f is not None else [None] * len(model_f.ordered_parameters())
        owner.last_flat_grads = (g_c, g_f)
        return (d_d if ctx.needs_input_grad[0] else None, d_o if ctx.needs_input_grad[1] else None, None, *grads_c, *grads_f)


def render_test(owner, model_c, model_f, rays_d, rays_o, eps_c, eps_sel, eps_f, prepared=None, u=None):
    """NeRF_Model.render_rays_test (model/mc_nerf.py:648-680): no jitter, step_r = 1, no cap, no grad; "voxel" mode only queries the
    grid.  `prepared` = (packed_c, packed_f, barf_w) from an enclosing chunk loop (the weights do not change inside it).
    "pdf" mode: `u` [N, n_importance] are the sampler's draws (the caller passes linspace(0, 1) rows: a deterministic render)."""
    st, dev = owner.settings, rays_d.device
    flat_c, flat_f = model_c.flat_params(), model_f.flat_params()
    if prepared is None:
        prepared = (_packed(model_c, flat_c, st, dev), _packed(model_f, flat_f, st, dev), owner.emmbedding_xyz.barf_weights_on(1, dev, pad=10))
    packed_c, packed_f, barf_w = prepared
    rays = Rays(d=rays_d.contiguous(), o=rays_o.contiguous(), barf_w=barf_w)
    rows = bounds_rows(owner, rays, None)
    coarse = coarse_pass(owner, model_c, flat_c, packed_c, rays, None, eps_c, prune=True, rows=rows)
    _, _, _, w_sel, wmax = run_pass(coarse, st, rays, eps_sel=eps_sel)
    fine = fine_pass(owner, model_f, flat_f, packed_f, rays, None, w_sel, wmax, eps_f, u, None, train=False, rows=rows)
    return run_pass(fine, st, rays, want_depth=True)[:3]                    # rgb, depth, opacity


class RaygenFn(torch.autograd.Function):
    """rays_d, rays_o = f(pose[3,4], kinv[3,3]) for the given pixel ids of one camera."""

    @staticmethod
    def forward(ctx, pose, kinv, pix, W):
        pose = pose.contiguous().float()
        kinv = kinv.contiguous().float()
        pix = pix.contiguous()
        d, o = ops.raygen_fwd(pose, kinv, pix, W)
        ctx.save_for_backward(pose, kinv, pix)
        ctx.W = W
        return d, o

    @staticmethod
    def backward(ctx, g_d, g_o):
        pose, kinv, pix = ctx.saved_tensors
        d_pose, d_kinv = ops.raygen_bwd(pose, kinv, pix, ctx.W, g_d.contiguous(), g_o.contiguous())
        return d_pose, d_kinv, None, None


class RayBatchFn(torch.autograd.Function):
    """pix, rays_d, rays_o, gt = f(pose[C,3,4], kinv[C,3,3]; lens[C,2] | None) for a batch of K segments of consecutive rays, segment k
    of camera seg_cam[k], in one launch: ops.ray_batch_fwd (`cams_per_step` > 1), or with `lens` ops.lens_ray_batch_fwd, the same with
    per-camera radial lens distortion (`lens_model` = "radial", any K).  Differentiable wrt pose, kinv and lens; `pix` (injected, or
    drawn on the device when None) and `gt` (from `images` [C, H*W, 3|4] uint8, None without) are non-differentiable outputs.
    `lens` is the last input: without it the argument list is the pinhole op's."""

    @staticmethod
    def forward(ctx, pose, kinv, seg_cam, seg_start, H, W, images=None, pix=None, seed=None, lens=None):
        pose = pose.contiguous().float()
        kinv = kinv.contiguous().float()
        kw = dict(images=images, pix=None if pix is None else pix.contiguous(), seed=seed)
        if lens is None:
            pix, d, o, gt = ops.ray_batch_fwd(pose, kinv, seg_cam, seg_start, H, W, **kw)
            ctx.save_for_backward(pose, kinv, pix)
        else:
            lens = lens.contiguous().float()
            pix, d, o, gt = ops.lens_ray_batch_fwd(pose, kinv, lens, seg_cam, seg_start, H, W, **kw)
            ctx.save_for_backward(pose, kinv, pix, lens)
        ctx.table = (list(seg_cam), list(seg_start), W)
        ctx.mark_non_differentiable(*(t for t in (pix, gt) if t is not None))
        return pix, d, o, gt

    @staticmethod
    def backward(ctx, _g_pix, g_d, g_o, _g_gt):
        pose, kinv, pix, *lens = ctx.saved_tensors
        seg_cam, seg_start, W = ctx.table
        if lens:
            d_pose, d_kinv, d_lens = ops.lens_ray_batch_bwd(pose, kinv, lens[0], seg_cam, seg_start, W, pix, g_d.contiguous(), g_o.contiguous())
        else:
            d_pose, d_kinv, d_lens = (*ops.ray_batch_bwd(pose, kinv, seg_cam, seg_start, W, pix, g_d.contiguous(), g_o.contiguous()), None)
        return d_pose, d_kinv, None, None, None, None, None, None, None, d_lens


class CameraFn(torch.autograd.Function):
    """K, Kinv, pose, calib_pose, pix_intr, pix_extr = f(weights_pose, weights_pose_intr, weights_fx, weights_fy, weights_ux,
    weights_uy; calibration world points) for all cameras in one fused kernel each way (reference: model/mc_nerf.py:171-210,
    269-316 and the reprojection branch :147-152, 236-267).  wpts_intr / wpts_extr [C,P,3] may be None (pixels not wanted)."""

    @staticmethod
    def forward(ctx, wpose, wpose_intr, wfx, wfy, wux, wuy, H, W, wpts_intr=None, wpts_extr=None):
        args = [t.contiguous().float() for t in (wpose, wpose_intr, wfx, wfy, wux, wuy)]
        pts = [None if t is None else t.contiguous().float() for t in (wpts_intr, wpts_extr)]
        K, Kinv, pose, calib, pi, pe = ops.camera_fwd(*args, H, W, pts[0], pts[1])
        ctx.save_for_backward(*args)
        ctx.pts = pts
        ctx.hw = (H, W)
        ctx.set_materialize_grads(False)
        return K, Kinv, pose, calib, pi, pe

    @staticmethod
    def backward(ctx, dK, dKinv, dpose, dcalib, dpi, dpe):
        args = ctx.saved_tensors
        grads = ops.camera_bwd(*args, ctx.hw[0], ctx.hw[1], dK, dKinv, dpose, dcalib, ctx.pts[0], ctx.pts[1], dpi, dpe)
        return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[:6])) + (None, None, None, None)


class TrainLossFn(torch.autograd.Function):
    """MC_NeRF_Loss.forward (model/loss.py:13-31) for the NeRF stages' keys {"intr", "rgb"} as ONE launch: value and every
    gradient; backward scales the saved gradients by the upstream scalar (one launch)."""

    @staticmethod
    def forward(ctx, pd, pt_gt, rgb_c, rgb_f, gt, H, W, normalise):
        cf = lambda t: None if t is None else t.contiguous().float()
        pd, pt_gt, rgb_c, rgb_f, gt = cf(pd), cf(pt_gt), cf(rgb_c), cf(rgb_f), cf(gt)
        out, d_pd, d_c, d_f = ops.train_loss(pd, pt_gt, H, W, normalise, rgb_c, rgb_f, gt)
        ctx.grads = (d_pd, d_c, d_f)
        ctx.parts = out
        return out[0]

    @staticmethod
    def backward(ctx, g):
        d_pd, d_c, d_f = ctx.grads
        ops.scale3_(d_pd, d_c, d_f, g.contiguous().float().reshape(1))
        ctx.grads = None
        return d_pd, None, d_c, d_f, None, None, None, None


class TrainLossCalibFn(torch.autograd.Function):
    """TrainLossFn with the per-camera colour calibration (csrc/color_calib.hip): value and every gradient, d weights_color
    included, in ONE launch; backward scales the saved gradients by the upstream scalar on the device (no host sync).  `pd` / `pt_gt`
    may be None (no reprojection term: get_rgb_loss_calibrated)."""

    @staticmethod
    def forward(ctx, pd, pt_gt, rgb_c, rgb_f, gt, color_w, seg_cam, seg_start, H, W, normalise, reg):
        cf = lambda t: None if t is None else t.contiguous().float()
        pd, pt_gt, rgb_c, rgb_f, gt, color_w = cf(pd), cf(pt_gt), cf(rgb_c), cf(rgb_f), cf(gt), cf(color_w)
        out, d_pd, d_c, d_f, d_color = ops.train_loss_calib(pd, pt_gt, H, W, normalise, rgb_c, rgb_f, gt, color_w, seg_cam, seg_start, reg)
        ctx.grads = (d_pd, d_c, d_f, d_color)
        ctx.parts = out
        return out[0]

    @staticmethod
    def backward(ctx, g):
        d_pd, d_c, d_f, d_color = ctx.grads
        g = g.contiguous().float().reshape(1)
        ops.scale3_(d_pd, d_c, d_f, g)
        ops.scale3_(None, d_color, None, g)
        ctx.grads = None
        return d_pd, None, d_c, d_f, None, d_color, None, None, None, None, None, None


class MaskLossFn(torch.autograd.Function):
    """weight * (mean (fg_c - alpha)^2 + mean (fg_f - alpha)^2) (csrc/mask.hip), value and both gradients in ONE launch of
    the extension library; backward scales the saved gradients by the upstream scalar on the device.  `fg_f` may be None (only_coarse);
    `alpha` [n] is a constant.  An empty batch is a zero that carries no gradient."""

    @staticmethod
    def forward(ctx, fg_c, fg_f, alpha, weight):
        cf = lambda t: None if t is None else t.contiguous().float().reshape(-1)
        ctx.shapes = (fg_c.shape, None if fg_f is None else fg_f.shape)
        fg_c, fg_f, alpha = cf(fg_c), cf(fg_f), cf(alpha)
        ctx.grads = None
        if fg_c.numel() == 0:
            return fg_c.new_zeros(())
        out, d_c, d_f = ops.mask_loss(fg_c, fg_f, alpha, weight)
        ctx.grads = (d_c, d_f)
        ctx.parts = out
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if ctx.grads is None:
            return None, None, None, None
        d_c, d_f = ctx.grads
        ops.scale3_(None, d_c, d_f, g.contiguous().float().reshape(1))
        ctx.grads = None
        return d_c.reshape(ctx.shapes[0]), None if d_f is None else d_f.reshape(ctx.shapes[1]), None, None


class DepthLossFn(torch.autograd.Function):
    """weight * (1 / max(n_valid, 1)) sum_valid [(s(zexp_c) - s(d_gt))^2 + (s(zexp_f) - s(d_gt))^2], s(z) = (z - near) / (far - near)
    (csrc/depth.hip), value and both gradients in the geometry library's two launches; backward scales the saved gradients
    by the upstream scalar on the device.  `zexp_f` may be None (only_coarse); `d_gt` [n] is a constant, valid where finite and > 0.
    An empty batch is a zero that carries no gradient; a batch without a valid target is an exact zero with exact-zero gradients."""

    @staticmethod
    def forward(ctx, zexp_c, zexp_f, d_gt, near, far, weight):
        cf = lambda t: None if t is None else t.contiguous().float().reshape(-1)
        ctx.shapes = (zexp_c.shape, None if zexp_f is None else zexp_f.shape)
        zexp_c, zexp_f, d_gt = cf(zexp_c), cf(zexp_f), cf(d_gt)
        ctx.grads = None
        if zexp_c.numel() == 0:
            return zexp_c.new_zeros(())
        out, d_c, d_f = ops.depth_loss(zexp_c, zexp_f, d_gt, near, far, weight)
        ctx.grads = (d_c, d_f)
        ctx.parts = out
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if ctx.grads is None:
            return None, None, None, None, None, None
        d_c, d_f = ctx.grads
        ops.scale3_(None, d_c, d_f, g.contiguous().float().reshape(1))
        ctx.grads = None
        return d_c.reshape(ctx.shapes[0]), None if d_f is None else d_f.reshape(ctx.shapes[1]), None, None, None, None


class ReprojLossFn(torch.autograd.Function):
    """MC_NeRF_Loss.get_reproject_loss (model/loss.py:45-58) as one kernel each way."""

    @staticmethod
    def forward(ctx, pd, gt, H, W):
        pd, gt = pd.contiguous().float(), gt.contiguous().float()
        ctx.save_for_backward(pd, gt)
        ctx.hw = (H, W)
        return ops.reproj_loss_fwd(pd, gt, H, W)

    @staticmethod
    def backward(ctx, dloss):
        pd, gt = ctx.saved_tensors
        return ops.reproj_loss_bwd(pd, gt, ctx.hw[0], ctx.hw[1], dloss.contiguous().float()), None, None, None
