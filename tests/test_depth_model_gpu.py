"""Depth supervision through the renderer, the models and the loss (sys_param key "depth_weight").  f32, small nets, 256
rays, 32 x 32 images; the configurations and launch lists are those of tests/test_render_passes_gpu.py.

  off is today    with the key absent or 0.0, `_geo.call` is never reached, the launch list is today's, `last_expected_depth` is None,
                  and the two models' loss and composite-backward outputs are torch.equal; their parameter gradients differ by the
                  order of the weight-gradient kernels' float atomics only (see the test);
  feature on      the list is today's plus geo_depth_fwd after each composite_fwd (after front_weight / distortion_fwd when those are
                  on), with geo_composite_bwd_z in place of each composite backward; rgb_c / rgb_f are the feature-off call's bits;
  gradients       parameter gradients of sum zexp_c p + sum zexp_f q (random p, q) against fp32 autograd through the oracle's render
                  (its out_c / out_f weighted by its own sigma2weights), per tensor relative to its own largest entry, at the f32 row of
                  PARITY_GATES as tests/test_distortion_model_gpu.py applies it -- uncapped, capped and only_coarse;
  combinations    with mask_weight and dist_weight on together, with fine_sampler "pdf", with coarse_sampler "voxel" past the warm-up
                  and with only_coarse: one backward with every gradient equals the sum of one backward each;
  MC_Model        one NeRF-stage step at cams_per_step 1 and 3 on the blob scene with its depth images attached: the targets are the
                  indexed values, the loss is the feature-off step's + the fp64 term of `last_expected_depth` and the targets; two
                  steps are finite;
  refusals        an image set without depth, a host float stack (ValueError naming depth_weight), a CPU model (McnerfError);
  retained graph  a second backward on a retained graph is still refused.
"""
import statistics

import pytest
import torch

import depth_ref as Z
import test_render_passes_gpu as P
from __graft_entry__ import PARITY_GATES, gradient_errors, reorder_noise
from conftest import make_sys_param
from mc_nerf_amd import synthetic as S

pytestmark = pytest.mark.gpu

N_RAYS = P.N_RAYS
DEPTH_MODES = ("uncapped", "capped", "pdf", "voxel_pruned", "only_coarse")


def _model(dev, mode, **extra):
    from mc_nerf_amd.model import NeRF_Model
    torch.manual_seed(1)               # (identical parameters in every model of one mode)
    sp = S.make_sys_param(dev, batch=N_RAYS, H=32, W=32, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision="f32", **P.MODES[mode][0], **extra)
    return NeRF_Model(sp).to(dev)


def _recorders(monkeypatch):
    from mc_nerf_amd import _ext, _geo, _lib, _reg
    seen = []
    for mod in (_lib, _ext, _reg, _geo):
        monkeypatch.setattr(mod, "call", (lambda real: lambda name, *a: (seen.append(name), real(name, *a))[1])(mod.call))
    return seen


def _depth_list(lst, mask=False, dist=False):
    out = []
    for n in lst:
        out.append("geo_composite_bwd_z" if n == "composite_bwd" else n)
        if n == "composite_fwd":
            out += (["ext_front_weight"] if mask else []) + (["reg_distortion_fwd"] if dist else []) + ["geo_depth_fwd"]
    return out


def _step(m, mode, d, o, p=None, q=None, use=("rgb", "fg", "dist", "zexp"), **draws):
    """One train step whose loss is the sum of the parts named in `use` that the model has: the colour sums of
    test_render_passes_gpu._step, the plain sums of the front weights and of the distortion terms, sum zexp_c p + sum zexp_f q."""
    rgb_c, rgb_f = P._train(m, mode, d, o, **draws)
    m.zero_grad(set_to_none=True)
    loss = 0.0
    if "rgb" in use:
        loss = rgb_c.sum() if rgb_f is None else rgb_c.sum() + rgb_f.sum()
    for name, last, wc, wf in (("fg", m.last_front_weight, None, None), ("dist", m.last_distortion, None, None), ("zexp", m.last_expected_depth, p, q)):
        if name in use and last is not None:
            c, f = last
            loss = loss + (c * (1.0 if wc is None else wc)).sum() + (0.0 if f is None else (f * (1.0 if wf is None else wf)).sum())
    loss.backward()
    return rgb_c, rgb_f, loss.detach()


# ---------------------------------------------------------------------------------------------------------------- off / on
@pytest.mark.parametrize("mode", DEPTH_MODES)
def test_off_is_today(gpu_device, monkeypatch, mode):
    """Key absent against key 0.0, same parameters and draws.  torch.equal: the loss, and the composite backward's output of every pass
    (what the feature could change: the operand the dX chain and the weight-gradient kernels start from).  The parameter gradients
    themselves are NOT reproducible bit for bit on this code base, with or without this feature: the weight-gradient kernels flush their
    accumulators with float atomics (csrc/mlp_dw.hip), whose order differs from launch to launch -- measured here between the two
    models: 2.2e-6 .. 2.6e-6 of a tensor's largest entry in every mode.  They are held to the reference's own reorder noise instead (the figure the
    PARITY_GATES are multiples of, tests/golden: what fp32 gradients do when only the order of their sums changes), with no multiplier."""
    from mc_nerf_amd import ops
    dev = gpu_device
    absent, zero = _model(dev, mode), _model(dev, mode, depth_weight=0.0)
    d, o = P._rays(dev)
    dr = P._draws(absent, dev)
    out = []
    for m in (absent, zero):
        _step(m, mode, d, o, **dr)                          # (a model's first call also lays out its flat parameter buffers)
        seen, d_outs = _recorders(monkeypatch), []
        monkeypatch.setattr(ops, "mlp_bwd", (lambda real: lambda *a, **kw: (d_outs.append(a[9].clone()), real(*a, **kw))[1])(ops.mlp_bwd))
        torch.manual_seed(123)                              # (capped: the cap's random subset is keyed from torch's device generator)
        _, _, loss = _step(m, mode, d, o, **dr)
        monkeypatch.undo()
        assert seen == P._names(P.TRAIN[mode], "f32") and not [n for n in seen if n.startswith("mcnerf_geo_")]
        assert m.last_expected_depth is None and m.settings.want_zexp is False
        out.append((loss, d_outs, {n: prm.grad.detach().clone() for n, prm in m.named_parameters() if prm.grad is not None}))
    (loss_a, d_a, grads_a), (loss_z, d_z, grads_z) = out
    assert torch.equal(loss_a, loss_z) and list(grads_a) == list(grads_z) and len(grads_a) >= 16
    assert len(d_a) == len(d_z) == (1 if mode == "only_coarse" else 2)
    for x, y in zip(d_a, d_z):
        assert x.dim() == 3 and x.shape[-1] == 4 and torch.equal(x.view(torch.int32), y.view(torch.int32))
    n_worst, _ = reorder_noise()
    rel = {n: float((grads_a[n] - grads_z[n]).abs().max()) / max(float(grads_a[n].abs().max()), 1e-30) for n in grads_a}
    print(f"[off is today, {mode}] parameter gradients, two models: worst {max(rel.values()):.2e} of the tensor's largest entry (bar {n_worst:.1e})")
    assert max(rel.values()) <= n_worst, max(rel, key=rel.get)


@pytest.mark.parametrize("mode", DEPTH_MODES)
def test_feature_on_adds_depth_fwd_and_swaps_the_composite_backward(gpu_device, monkeypatch, mode):
    dev = gpu_device
    on, off = _model(dev, mode, depth_weight=0.5), _model(dev, mode)
    d, o = P._rays(dev)
    dr = P._draws(on, dev)
    _step(on, mode, d, o, **dr)
    seen = _recorders(monkeypatch)
    torch.manual_seed(123)
    rgb_c, rgb_f, _ = _step(on, mode, d, o, **dr)
    assert seen == P._names(_depth_list(P.TRAIN[mode]), "f32")
    monkeypatch.undo()
    zexp_c, zexp_f = on.last_expected_depth
    assert zexp_c.shape == (N_RAYS,) and zexp_c.requires_grad and bool(torch.isfinite(zexp_c).all())
    assert float(zexp_c.detach().min()) >= 0.0 and float(zexp_c.detach().max()) <= float(on.far) + float(on.far - on.near) / on.samples_c + 1e-3
    assert (zexp_f is None) == (mode == "only_coarse") and (zexp_f is None or (zexp_f.shape == (N_RAYS,) and zexp_f.requires_grad))
    assert on.last_front_weight is None and on.last_distortion is None
    # the same bits as the feature-off call on the same draws (voxel mode: each model's grid has seen the same two steps)
    P._step(off, mode, d, o, **dr)
    torch.manual_seed(123)
    ref_c, ref_f = P._train(off, mode, d, o, **dr)
    assert torch.equal(rgb_c, ref_c) and (rgb_f is None or torch.equal(rgb_f, ref_f))
    # an empty batch: empty, graph-free terms
    e = on.render_rays_train(d[:0], o[:0], P.MODES[mode][1], 1.0, only_coarse=P.MODES[mode][2])
    assert e[0].shape == (0, 3) and on.last_expected_depth[0].shape == (0,)
    assert (on.last_expected_depth[1] is None) == (mode == "only_coarse")


@pytest.mark.parametrize("mode", ["uncapped", "pdf", "only_coarse"])
def test_with_mask_and_distortion_one_backward_carries_all(gpu_device, monkeypatch, mode):
    dev = gpu_device
    m = _model(dev, mode, depth_weight=0.5, dist_weight=0.5, mask_weight=0.5)
    d, o = P._rays(dev)
    dr = P._draws(m, dev)
    _step(m, mode, d, o, **dr)
    seen = _recorders(monkeypatch)
    _step(m, mode, d, o, **dr)
    assert seen == P._names(_depth_list(P.TRAIN[mode], mask=True, dist=True), "f32")
    assert not {"mcnerf_ext_composite_bwd_front", "mcnerf_reg_composite_bwd_w", "mcnerf_composite_bwd"} & set(seen)
    assert m.last_distortion is not None and m.last_front_weight is not None and m.last_expected_depth is not None
    nets = (m.nerf_coarse,) if mode == "only_coarse" else (m.nerf_coarse, m.nerf_fine)
    assert all(prm.grad is not None and bool(torch.isfinite(prm.grad).all()) for net in nets for prm in net.parameters())


# ---------------------------------------------------------------------------------------------------------------- gradients
def _oracle_cfg(mode):
    from oracle import mcnerf_oracle as O
    kw = P.MODES[mode][0]
    return O.RenderCfg(samples=kw["samples"], scale=kw["scale"], coarse=O.NetCfg(4, 32, (2,)), fine=O.NetCfg(8, 64, (4,)))


def _oracle_zexp(O, z, sigma, eps):
    """The expected depth on the oracle's own weights on depths z [N,S] (fp32 torch)."""
    return (O.sigma2weights(O.deltas_of(z), sigma, eps) * z).sum(dim=1)


@pytest.mark.parametrize("mode", ["uncapped", "capped", "only_coarse"])
def test_expected_depth_gradients_against_the_oracle(gpu_device, mode):
    """f32 mode: parameter gradients of sum zexp_c p + sum zexp_f q against fp32 autograd through the oracle's render.  Bars: the
    multiples of the reference's reorder noise of test_full_size_gradient_golden (the f32 row of PARITY_GATES)."""
    from oracle import mcnerf_oracle as O
    from mc_nerf_amd.model import NeRF_Model
    dev = gpu_device
    cfg = _oracle_cfg(mode)
    only_coarse = P.MODES[mode][2]
    pc, pf = O.init_params(cfg.coarse, 1), O.init_params(cfg.fine, 2)
    for prm in list(pc.values()) + list(pf.values()):
        prm.requires_grad_(True)
    m = NeRF_Model(make_sys_param(cfg, str(dev), batch=N_RAYS, precision="f32", depth_weight=1.0)).to(dev)
    m.nerf_coarse.load_state_dict({k: v.detach() for k, v in pc.items()})
    m.nerf_fine.load_state_dict({k: v.detach() for k, v in pf.items()})
    d, o = P._rays(dev)
    dr = P._draws(m, dev)
    g = torch.Generator().manual_seed(9)
    p, q = torch.randn(N_RAYS, generator=g), torch.randn(N_RAYS, generator=g)
    c = {k: v.cpu() for k, v in dr.items()}
    zc, zf = O._grids(cfg)
    cap_perm = None
    if not only_coarse:                 # the cap's permutation is over the selected list: its length first (model/mc_nerf.py:631)
        with torch.no_grad():
            z_c = zc.unsqueeze(0) + c["jitter"]
            sig_c = O.inference(pc, cfg.coarse, cfg, 1.0, o.cpu(), d.cpu(), z_c, c["eps_c"])[1]
            n_sel = O.select_fine(O.sigma2weights(O.deltas_of(z_c), sig_c, c["eps_sel"]), cfg).shape[0]
        cap_perm = torch.randperm(n_sel, generator=g)
        assert (n_sel > N_RAYS * cfg.max_fine_per_ray) == (mode == "capped")
    # the oracle
    r = O.render_rays_train(pc, pf, cfg, d.cpu(), o.cpu(), 1.0, c["jitter"], c["eps_c"], c["eps_sel"], c["eps_f"], cap_perm=cap_perm, only_coarse=only_coarse)
    ref_c = _oracle_zexp(O, zc.unsqueeze(0) + c["jitter"], r["out_c"][..., 0], c["eps_c"])
    loss = (ref_c * p).sum()
    if not only_coarse:
        ref_f = _oracle_zexp(O, zf.unsqueeze(0) + c["jitter"], r["out_f"][..., 0], c["eps_f"])
        loss = loss + (ref_f * q).sum()
    loss.backward()
    # the HIP path: the depth terms alone (d_rgb arrives as zeros)
    m.render_rays_train(d, o, 0, 1.0, only_coarse=only_coarse, cap_perm=cap_perm, **dr)
    zexp_c, zexp_f = m.last_expected_depth
    ((zexp_c * p.to(dev)).sum() + (0.0 if zexp_f is None else (zexp_f * q.to(dev)).sum())).backward()
    assert float(ref_c.detach().std()) > 1e-2                           # the term is live on these rays
    assert float((zexp_c.detach().cpu() - ref_c.detach()).abs().max()) < 1e-4 * 8.0
    assert only_coarse or float((zexp_f.detach().cpu() - ref_f.detach()).abs().max()) < 1e-4 * 8.0
    nets, refs = ((m.nerf_coarse,), (pc,)) if only_coarse else ((m.nerf_coarse, m.nerf_fine), (pc, pf))
    errs = gradient_errors(nets, refs)
    assert len(errs) == (16 if only_coarse else 40)                    # (coarse 2 x 4 + 8 tensors, fine 2 x 8 + 8)
    for net, ref in zip(nets, refs):    # the term does not depend on the colour head: exactly zero there, in the oracle and here
        for k, prm in net.named_parameters():
            assert (float(prm.grad.abs().max()) > 0.0) == (float(ref[k].grad.abs().max()) > 0.0) == (not k.startswith("sh.")), k
    n_worst, n_median = reorder_noise()
    _, k_worst, k_median = PARITY_GATES["f32"]
    worst_key = max(errs, key=errs.get)
    e_worst, e_median = errs[worst_key], statistics.median(errs.values())
    print(f"[expected-depth gradients, {mode}] worst {e_worst:.2e} ({worst_key}; gate {k_worst:g} x {n_worst:.1e}), median {e_median:.2e} (gate {k_median:g} x {n_median:.1e})")
    assert e_worst < k_worst * n_worst and e_median < k_median * n_median


@pytest.mark.parametrize("mode, extra", [("uncapped", dict(mask_weight=1.0, dist_weight=1.0)), ("pdf", {}), ("voxel_pruned", {}), ("only_coarse", {}),
                                         ("pdf", dict(mask_weight=1.0, dist_weight=1.0))])
def test_one_backward_with_every_gradient_is_the_sum_of_one_each(gpu_device, mode, extra):
    """Where the oracle has no render: d (rgb + fg + dist + zexp terms) = the sum of a backward each, the first from ONE backward through
    composite_bwd_z with every upstream gradient, the others with one part of the loss each (the rest arrives as zeros)."""
    dev = gpu_device
    g = torch.Generator().manual_seed(9)
    p, q = torch.randn(N_RAYS, generator=g).to(dev), torch.randn(N_RAYS, generator=g).to(dev)
    d, o = P._rays(dev)
    parts = ["rgb", "zexp"] + (["fg", "dist"] if extra else [])
    grads = {}
    for which in ["all"] + parts:
        m = _model(dev, mode, depth_weight=1.0, **extra)                       # (a step changes the voxel grid: one model each)
        dr = P._draws(m, dev)
        _step(m, mode, d, o, p, q, use=tuple(parts) if which == "all" else (which,), **dr)
        grads[which] = {n: prm.grad.detach().clone() for n, prm in m.named_parameters() if prm.grad is not None}
    for n, both in grads["all"].items():
        want = sum(grads[part][n] for part in parts)
        assert (float(grads["zexp"][n].abs().max()) > 0.0) == (".sh." not in n), n        # (the term does not depend on the colour head)
        assert float((both - want).abs().max()) <= 1e-4 * float(want.abs().max()) + 1e-12, n


# ---------------------------------------------------------------------------------------------------------------- MC_Model
STAGE = "GLOBAL_OPTIM_EPOCH"
H = W = 32
CAMS = [5, 0, 5]
_SCENE = {}


def _scene(dev):
    """The blob scene's images (uint8) and depth images of the synthetic rig, rendered once."""
    if not _SCENE:
        sp = S.make_sys_param(dev, samples=32, scale=2, batch=N_RAYS, H=H, W=W)
        pose, K = sp["gt_pose"].to(dev), sp["intr_mat"][0].to(dev)
        rgb = S.blob_scene_images(pose, K, H, W)
        _SCENE["u8"] = rgb.mul(255.0).round().to(torch.uint8).contiguous()
        _SCENE["depth"] = S.blob_scene_depth_images(pose, K, H, W).contiguous()
    return _SCENE["u8"], _SCENE["depth"]


def _mc_setup(dev, K, lam, with_depth=True, **extra):
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model
    if K > 1:
        extra["cams_per_step"] = K
    if lam:
        extra["depth_weight"] = lam
    sp = S.make_sys_param(dev, samples=32, scale=2, batch=N_RAYS, H=H, W=W, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision="f32", **extra)
    torch.manual_seed(3)
    model = MC_Model(sp).to(dev)
    S.init_cameras_near_gt(model)
    u8, depth = _scene(dev)
    images = DeviceImageSet(u8, H, W, depth=depth if with_depth else None)
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    return sp, model, (images, torch.tensor(CAMS[:K]), wpts, pts, wpts, pts)


@pytest.mark.parametrize("K", [1, 3])
def test_mc_model_step_adds_the_depth_term(gpu_device, K):
    from mc_nerf_amd import ops
    from mc_nerf_amd.model import MC_NeRF_Loss
    dev, lam = gpu_device, 0.7
    seg = ops.ray_segments(N_RAYS, K)
    g = torch.Generator().manual_seed(21)
    pix = torch.cat([torch.randperm(H * W, generator=g)[:b - a] for a, b in zip(seg, seg[1:])]).to(dev)
    out = {}
    for w in (0.0, lam):
        sp, model, data = _mc_setup(dev, K, w)
        model.sample_pixels_multi = lambda npix, seg_start: pix
        model.sample_pixels = lambda npix: pix
        torch.manual_seed(17)                               # the renderer's draws: the same in both steps
        loss_dict, *_ = model(data, 20, STAGE, 0.5)
        crit = MC_NeRF_Loss(sp)
        loss = crit(loss_dict, STAGE)
        loss.backward()
        assert crit.global_step == 1
        out[w] = (loss_dict, float(loss.detach()), model.weights_pose.grad.detach().clone(), model.nerf.last_expected_depth, data[0])
    (off_dict, off_loss, off_grad, off_last, _), (on_dict, on_loss, on_grad, last, images) = out[0.0], out[lam]
    assert "depth" not in off_dict and off_last is None and set(on_dict) == set(off_dict) | {"depth"}
    assert torch.equal(on_dict["rgb"][0], off_dict["rgb"][0]) and torch.equal(on_dict["rgb"][1], off_dict["rgb"][1])
    zexp_c, zexp_f, d_gt = on_dict["depth"]
    assert zexp_c is last[0] and zexp_f is last[1] and zexp_c.shape == (N_RAYS,) and zexp_f.shape == (N_RAYS,)
    # the gathered targets: the indexed value where it is a measurement, else 0
    cam_of = torch.cat([torch.full((b - a,), c, dtype=torch.int64) for c, a, b in zip(CAMS[:K], seg, seg[1:])]).to(dev)
    stored = images.depth[cam_of, pix]
    assert torch.equal(d_gt, torch.where(torch.isfinite(stored) & (stored > 0), stored, torch.zeros_like(stored)))
    assert torch.equal(d_gt, ops.gather_depth(images.depth, CAMS[:K], seg, pix))
    n_valid = int((d_gt > 0).sum())
    assert 10 < n_valid < N_RAYS                            # the blobs cover part of every image: both kinds of pixel are drawn
    term, m, nv, _, _ = Z.loss64(zexp_c.detach().cpu(), zexp_f.detach().cpu(), d_gt.cpu(), sp["near"], sp["far"], lam)
    print(f"[depth step, K = {K}] loss {on_loss:.6f} = {off_loss:.6f} + {term:.6f} ({nv} of {N_RAYS} rays have a target)")
    assert nv == n_valid and term > 1e-3 and abs(on_loss - (off_loss + term)) <= 2e-6 * max(1.0, abs(off_loss + term))
    rows = sorted(set(CAMS[:K]))
    assert float(on_grad[rows].abs().max()) > 0.0 and float((on_grad - off_grad)[rows].abs().max()) > 1e-6 * float(off_grad.abs().max())
    others = [c for c in range(on_grad.shape[0]) if c not in rows]
    assert torch.equal(on_grad[others], off_grad[others])


@pytest.mark.parametrize("K", [1, 3])
def test_two_steps_are_finite(gpu_device, K):
    from mc_nerf_amd.model import MC_NeRF_Loss
    dev = gpu_device
    sp, model, data = _mc_setup(dev, K, 0.5)
    crit = MC_NeRF_Loss(sp)
    opt = torch.optim.SGD([prm for prm in model.parameters() if prm.requires_grad], lr=1e-4)
    torch.manual_seed(4)
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        loss_dict, *_ = model(data, 20, STAGE, 0.5)
        loss = crit(loss_dict, STAGE)
        loss.backward()
        assert bool(torch.isfinite(loss)) and "depth" in loss_dict
        assert all(bool(torch.isfinite(prm.grad).all()) for prm in model.parameters() if prm.grad is not None)
        opt.step()


def test_step_refusals(gpu_device):
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import MC_Model
    dev = gpu_device
    _, model, data = _mc_setup(dev, 1, 0.5, with_depth=False)
    with pytest.raises(ValueError, match="depth_weight.*without depth"):
        model(data, 20, STAGE, 0.5)
    with pytest.raises(ValueError, match="depth_weight.*host float image stack"):
        model((torch.rand(1, H * W, 3), *data[1:]), 20, STAGE, 0.5)
    _, model3, data3 = _mc_setup(dev, 3, 0.5, with_depth=False)
    with pytest.raises(ValueError, match="depth_weight"):
        model3(data3, 20, STAGE, 0.5)
    sp = S.make_sys_param("cpu", samples=8, scale=2, batch=16, H=8, W=8, coarse=(2, 32, [1]), fine=(2, 32, [1]), depth_weight=0.5)
    cpu = MC_Model(sp)
    S.init_cameras_near_gt(cpu)
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    with pytest.raises(McnerfError, match="depth_weight"):
        cpu((torch.rand(1, 64, 3), torch.tensor([0]), wpts, pts, wpts, pts), 20, STAGE, 0.6)
    m = _model("cpu", "uncapped", depth_weight=0.5)
    d, o = P._rays(torch.device("cpu"))
    with pytest.raises(McnerfError, match="depth_weight"):
        m.render_rays_train(d, o, 0, 1.0)


def test_get_depth_loss_serves_a_loop_that_drives_the_renderer(gpu_device):
    from mc_nerf_amd.model import MC_NeRF_Loss
    dev = gpu_device
    m = _model(dev, "uncapped", depth_weight=0.25)
    d, o = P._rays(dev)
    m.render_rays_train(d, o, 0, 1.0, **P._draws(m, dev))
    zexp_c, zexp_f = m.last_expected_depth
    target = S.blob_scene_depth(d, o, 1.0, 8.0, 384)
    crit = MC_NeRF_Loss(S.make_sys_param(dev, batch=N_RAYS, H=32, W=32, depth_weight=0.25))
    v = crit.get_depth_loss([zexp_c, zexp_f, target], m.near, m.far)
    want = Z.loss64(zexp_c.detach().cpu(), zexp_f.detach().cpu(), target.cpu(), m.near, m.far, 0.25)[0]
    assert abs(float(v.detach()) - want) <= 2e-6 * max(1.0, want) and want > 0.0
    v2 = crit.get_depth_loss([zexp_c, zexp_f, target], m.near, m.far, weight=0.5)
    assert abs(float(v2.detach()) - 2.0 * want) <= 4e-6 * max(1.0, want)
    v.backward()
    assert all(prm.grad is not None and bool(torch.isfinite(prm.grad).all()) for prm in m.nerf_fine.parameters())


def test_second_backward_through_a_retained_graph_is_still_refused(gpu_device):
    from mc_nerf_amd._lib import McnerfError
    dev = gpu_device
    m = _model(dev, "uncapped", depth_weight=0.5)
    d, o = P._rays(dev)
    rgb_c, rgb_f = m.render_rays_train(d, o, 0, 1.0)
    zexp_c, zexp_f = m.last_expected_depth
    loss = rgb_c.sum() + rgb_f.sum() + zexp_c.sum() + zexp_f.sum()
    loss.backward(retain_graph=True)
    n_free = sum(len(v) for v in m.ws_pool.free.values())
    with pytest.raises(McnerfError, match="ran twice"):
        loss.backward()
    assert sum(len(v) for v in m.ws_pool.free.values()) == n_free          # nothing was pushed a second time
