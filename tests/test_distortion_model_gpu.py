"""The distortion loss through the renderer, the models and the loss (sys_param key "dist_weight").  Small nets, 256 rays,
32 x 32 images; the configurations and launch lists are those of tests/test_render_passes_gpu.py.

  feature off     with the key absent or 0.0, `_reg.call` is never reached and the train step's launch list is today's (`_lib.call`,
                  `_ext.call` and `_reg.call` are all recorded);
  feature on      the list is today's plus distortion_fwd after each composite_fwd, with composite_bwd_w in place of each
                  composite_bwd (uncapped, capped, pdf, voxel-pruned, only_coarse; f32 and f16x3); with mask_weight on as well:
                  front_weight then distortion_fwd, and ONE composite_bwd_w per pass;
  same bits       rgb_c / rgb_f are torch.equal to the feature-off call's on the same draws;
  gradients       parameter gradients of sum dist_c p + sum dist_f q (random p, q) against fp32 autograd through the oracle's render
                  (its out_c / out_f weighted by its own sigma2weights, the term in the prefix form), f32 mode, per tensor relative to
                  its own largest entry, at the gates test_front_weight_gradients_against_the_oracle uses -- uncapped, capped and
                  only_coarse; in pdf and voxel-pruned mode one backward with the rgb and dist gradients equals the sum of two
                  backwards with one each;
  MC_Model        one joint-stage step at cams_per_step 1 and 3: the loss is the feature-off step's + the fp64 term of
                  `last_distortion`, weights_pose receives a gradient that the term changes;
  refusals        a CPU model with the key on raises McnerfError naming dist_weight.
"""
import statistics

import pytest
import torch

import distortion_ref as D
import test_render_passes_gpu as P
from __graft_entry__ import PARITY_GATES, gradient_errors, reorder_noise
from conftest import make_sys_param
from mc_nerf_amd import synthetic as S

pytestmark = pytest.mark.gpu

N_RAYS = P.N_RAYS
DIST_MODES = ("uncapped", "capped", "pdf", "voxel_pruned", "only_coarse")
CASES = [(mode, precision) for mode in DIST_MODES for precision in P.PRECISIONS]


def _model(dev, mode, precision, **extra):
    from mc_nerf_amd.model import NeRF_Model
    torch.manual_seed(1)               # (identical parameters in every model of one mode and precision)
    sp = S.make_sys_param(dev, batch=N_RAYS, H=32, W=32, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision=precision, **P.MODES[mode][0], **extra)
    return NeRF_Model(sp).to(dev)


def _dist_list(lst, mask=False):
    out = []
    for n in lst:
        out.append("reg_composite_bwd_w" if n == "composite_bwd" else n)
        if n == "composite_fwd":
            out += ["ext_front_weight", "reg_distortion_fwd"] if mask else ["reg_distortion_fwd"]
    return out


def _recorders(monkeypatch):
    from mc_nerf_amd import _ext, _lib, _reg
    seen = []
    for mod in (_lib, _ext, _reg):
        monkeypatch.setattr(mod, "call", (lambda real: lambda name, *a: (seen.append(name), real(name, *a))[1])(mod.call))
    return seen


def _dist_step(m, mode, d, o, p=None, q=None, with_rgb=True, **draws):
    """One train step whose loss is (with_rgb: the colour sums of test_render_passes_gpu._step +) sum dist_c p + sum dist_f q (+ the
    plain sums of the front weights in mask mode)."""
    rgb_c, rgb_f = P._train(m, mode, d, o, **draws)
    m.zero_grad(set_to_none=True)
    loss = (rgb_c.sum() if rgb_f is None else rgb_c.sum() + rgb_f.sum()) if with_rgb else 0.0
    if m.last_distortion is not None:
        dist_c, dist_f = m.last_distortion
        loss = loss + (dist_c * (1.0 if p is None else p)).sum() + (0.0 if dist_f is None else (dist_f * (1.0 if q is None else q)).sum())
    if m.last_front_weight is not None:
        fg_c, fg_f = m.last_front_weight
        loss = loss + fg_c.sum() + (0.0 if fg_f is None else fg_f.sum())
    loss.backward()
    return rgb_c, rgb_f


@pytest.mark.parametrize("mode,precision", CASES)
@pytest.mark.parametrize("key", ["absent", "zero"])
def test_feature_off_never_reaches_the_regulariser_library(gpu_device, monkeypatch, mode, precision, key):
    dev = gpu_device
    m = _model(dev, mode, precision, **({} if key == "absent" else {"dist_weight": 0.0}))
    d, o = P._rays(dev)
    dr = P._draws(m, dev)
    _dist_step(m, mode, d, o, **dr)
    seen = _recorders(monkeypatch)
    _dist_step(m, mode, d, o, **dr)
    assert seen == P._names(P.TRAIN[mode], precision) and m.last_distortion is None
    assert not [n for n in seen if n.startswith(("mcnerf_reg_", "mcnerf_ext_"))]


@pytest.mark.parametrize("mode,precision", CASES)
def test_feature_on_adds_distortion_fwd_and_swaps_the_composite_backward(gpu_device, monkeypatch, mode, precision):
    dev = gpu_device
    on, off = _model(dev, mode, precision, dist_weight=0.5), _model(dev, mode, precision)
    d, o = P._rays(dev)
    dr = P._draws(on, dev)
    _dist_step(on, mode, d, o, **dr)
    seen = _recorders(monkeypatch)
    torch.manual_seed(123)             # (capped: the cap's random subset is keyed from torch's device generator)
    rgb_c, rgb_f = _dist_step(on, mode, d, o, **dr)
    assert seen == P._names(_dist_list(P.TRAIN[mode]), precision)
    monkeypatch.undo()
    dist_c, dist_f = on.last_distortion
    assert dist_c.shape == (N_RAYS,) and dist_c.requires_grad and float(dist_c.detach().min()) >= 0.0 and bool(torch.isfinite(dist_c).all())
    assert (dist_f is None) == (mode == "only_coarse") and (dist_f is None or (dist_f.shape == (N_RAYS,) and dist_f.requires_grad))
    assert on.last_front_weight is None
    # the same bits as the feature-off call on the same draws (voxel mode: each model's grid has seen the same two steps)
    P._step(off, mode, d, o, **dr)
    torch.manual_seed(123)
    ref_c, ref_f = P._train(off, mode, d, o, **dr)
    assert torch.equal(rgb_c, ref_c) and (rgb_f is None or torch.equal(rgb_f, ref_f))
    # an empty batch: empty, graph-free terms
    e = on.render_rays_train(d[:0], o[:0], P.MODES[mode][1], 1.0, only_coarse=P.MODES[mode][2])
    assert e[0].shape == (0, 3) and on.last_distortion[0].shape == (0,)
    assert (on.last_distortion[1] is None) == (mode == "only_coarse")


@pytest.mark.parametrize("mode,precision", [("uncapped", "f32"), ("pdf", "f16x3"), ("only_coarse", "f32")])
def test_with_mask_mode_one_backward_carries_both(gpu_device, monkeypatch, mode, precision):
    dev = gpu_device
    m = _model(dev, mode, precision, dist_weight=0.5, mask_weight=0.5)
    d, o = P._rays(dev)
    dr = P._draws(m, dev)
    _dist_step(m, mode, d, o, **dr)
    seen = _recorders(monkeypatch)
    _dist_step(m, mode, d, o, **dr)
    assert seen == P._names(_dist_list(P.TRAIN[mode], mask=True), precision)
    assert "mcnerf_ext_composite_bwd_front" not in seen and "mcnerf_composite_bwd" not in seen
    assert m.last_distortion is not None and m.last_front_weight is not None
    nets = (m.nerf_coarse,) if mode == "only_coarse" else (m.nerf_coarse, m.nerf_fine)          # (only_coarse: the fine net takes no part)
    assert all(prm.grad is not None and bool(torch.isfinite(prm.grad).all()) for net in nets for prm in net.parameters())


# ---------------------------------------------------------------------------------------------------------------- gradients
def _oracle_cfg(mode):
    from oracle import mcnerf_oracle as O
    kw = P.MODES[mode][0]
    return O.RenderCfg(samples=kw["samples"], scale=kw["scale"], coarse=O.NetCfg(4, 32, (2,)), fine=O.NetCfg(8, 64, (4,)))


def _oracle_dist(O, cfg, z, sigma, eps):
    """The term of the oracle's own weights on depths z [N,S] (fp32 torch, the prefix form of tests/distortion_ref.py)."""
    w = O.sigma2weights(O.deltas_of(z), sigma, eps)
    return D.dist_prefix(w, (z - cfg.near) * (1.0 / (cfg.far - cfg.near)))


@pytest.mark.parametrize("mode", ["uncapped", "capped", "only_coarse"])
def test_distortion_gradients_against_the_oracle(gpu_device, mode):
    """f32 mode: parameter gradients of sum dist_c p + sum dist_f q against fp32 autograd through the oracle's render.  Bars: the
    multiples of the reference's reorder noise of test_full_size_gradient_golden."""
    from oracle import mcnerf_oracle as O
    from mc_nerf_amd.model import NeRF_Model
    dev = gpu_device
    cfg = _oracle_cfg(mode)
    only_coarse = P.MODES[mode][2]
    pc, pf = O.init_params(cfg.coarse, 1), O.init_params(cfg.fine, 2)
    for prm in list(pc.values()) + list(pf.values()):
        prm.requires_grad_(True)
    m = NeRF_Model(make_sys_param(cfg, str(dev), batch=N_RAYS, precision="f32", dist_weight=1.0)).to(dev)
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
    ref_c = _oracle_dist(O, cfg, zc.unsqueeze(0) + c["jitter"], r["out_c"][..., 0], c["eps_c"])
    loss = (ref_c * p).sum()
    if not only_coarse:
        ref_f = _oracle_dist(O, cfg, zf.unsqueeze(0) + c["jitter"], r["out_f"][..., 0], c["eps_f"])
        loss = loss + (ref_f * q).sum()
    loss.backward()
    # the HIP path: the distortion terms alone (d_rgb arrives as zeros)
    m.render_rays_train(d, o, 0, 1.0, only_coarse=only_coarse, cap_perm=cap_perm, **dr)
    dist_c, dist_f = m.last_distortion
    ((dist_c * p.to(dev)).sum() + (0.0 if dist_f is None else (dist_f * q.to(dev)).sum())).backward()
    assert float(ref_c.detach().max()) > 1e-2                           # the term is live on these rays
    assert float((dist_c.detach().cpu() - ref_c.detach()).abs().max()) < 1e-4
    assert only_coarse or float((dist_f.detach().cpu() - ref_f.detach()).abs().max()) < 1e-4
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
    print(f"[distortion gradients, {mode}] worst {e_worst:.2e} ({worst_key}; gate {k_worst:g} x {n_worst:.1e}), median {e_median:.2e} (gate {k_median:g} x {n_median:.1e})")
    assert e_worst < k_worst * n_worst and e_median < k_median * n_median


@pytest.mark.parametrize("mode", ["pdf", "voxel_pruned"])
def test_one_backward_with_both_gradients_is_the_sum_of_two(gpu_device, mode):
    """Where the oracle has no render: d (rgb terms + dist terms) = d (rgb terms) + d (dist terms), the first from ONE backward through
    composite_bwd_w with both upstream gradients, the others from a backward each (the dist one with d_rgb = zeros)."""
    dev = gpu_device
    g = torch.Generator().manual_seed(9)
    p, q = torch.randn(N_RAYS, generator=g).to(dev), torch.randn(N_RAYS, generator=g).to(dev)
    d, o = P._rays(dev)
    grads = {}
    for which in ("both", "dist", "rgb"):
        m = _model(dev, mode, "f32", **({} if which == "rgb" else {"dist_weight": 1.0}))      # (a step changes the voxel grid: one model each)
        dr = P._draws(m, dev)
        _dist_step(m, mode, d, o, p, q, with_rgb=which != "dist", **dr)
        grads[which] = {n: prm.grad.detach().clone() for n, prm in m.named_parameters()}
    for n, both in grads["both"].items():
        want = grads["rgb"][n] + grads["dist"][n]
        assert (float(grads["dist"][n].abs().max()) > 0.0) == (".sh." not in n), n        # (the term does not depend on the colour head)
        assert float((both - want).abs().max()) <= 1e-4 * float(want.abs().max()) + 1e-12, n


# ---------------------------------------------------------------------------------------------------------------- MC_Model
STAGE = "GLOBAL_OPTIM_EPOCH"
H = W = 32
CAMS = [5, 0, 5]


def _mc_setup(dev, K, lam):
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model
    extra = {}
    if K > 1:
        extra["cams_per_step"] = K
    if lam:
        extra["dist_weight"] = lam
    sp = S.make_sys_param(dev, samples=32, scale=2, batch=N_RAYS, H=H, W=W, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision="f32", **extra)
    torch.manual_seed(3)
    model = MC_Model(sp).to(dev)
    S.init_cameras_near_gt(model)
    u8 = torch.randint(0, 256, (model.train_numb, H * W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    images = DeviceImageSet(u8.contiguous().to(dev), H, W)
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    return sp, model, (images, torch.tensor(CAMS[:K]), wpts, pts, wpts, pts)


@pytest.mark.parametrize("K", [1, 3])
def test_mc_model_step_adds_the_distortion_term(gpu_device, K):
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
        loss = MC_NeRF_Loss(sp)(loss_dict, STAGE)
        loss.backward()
        out[w] = (loss_dict, float(loss.detach()), model.weights_pose.grad.detach().clone(), model.nerf.last_distortion)
    (off_dict, off_loss, off_grad, off_last), (on_dict, on_loss, on_grad, last) = out[0.0], out[lam]
    assert "dist" not in off_dict and off_last is None and set(on_dict) == set(off_dict) | {"dist"}
    assert torch.equal(on_dict["rgb"][0], off_dict["rgb"][0]) and torch.equal(on_dict["rgb"][1], off_dict["rgb"][1])
    dist_c, dist_f = on_dict["dist"]
    assert dist_c is last[0] and dist_f is last[1] and dist_c.shape == (N_RAYS,) and dist_f.shape == (N_RAYS,)
    term = lam * float(dist_c.detach().double().mean() + dist_f.detach().double().mean())
    print(f"[distortion step, K = {K}] loss {on_loss:.6f} = {off_loss:.6f} + {term:.6f}")
    assert term > 1e-3 and abs(on_loss - (off_loss + term)) <= 2e-6 * max(1.0, abs(off_loss + term))
    rows = sorted(set(CAMS[:K]))
    assert float(on_grad[rows].abs().max()) > 0.0 and float((on_grad - off_grad)[rows].abs().max()) > 1e-6 * float(off_grad.abs().max())
    others = [c for c in range(on_grad.shape[0]) if c not in rows]
    assert torch.equal(on_grad[others], off_grad[others])


def test_a_cpu_model_with_the_key_on_refuses(gpu_device):
    from mc_nerf_amd._lib import McnerfError
    m = _model("cpu", "uncapped", "f32", dist_weight=0.5)
    d, o = P._rays(torch.device("cpu"))
    with pytest.raises(McnerfError, match="dist_weight"):
        m.render_rays_train(d, o, 0, 1.0)
