"""The scene box fitted to the voxel sigma cache through the renderer (sys_param key "ray_bounds_fit").  Small nets, 64 and
256 rays (tests/ray_bounds_ref.py::model_rays), a 16^3 grid over [-3.5, 3.5]^3.  Every comparison but one is equality.

  "fixed" and the absent key   the same bits as aabb mode without the key, with the fit library made unloadable;
  a grid left at sigma_init    every cell is occupied, the fitted box is the outer box: the train render (outputs and ray gradients) and
                               the test render are those of fixed aabb mode with that box bit for bit, threshold and pdf, "sample" and
                               "skip"; the parameter gradients (float atomics) lie among the fixed mode's own runs;
  a known blob                 last_scene_box is the restatement's box, last_ray_span / last_ray_hit are ops.ray_depths' on it as a tuple,
                               and the render is that of a fixed-box model given the six numbers;
  cadence                      the box's bits change at the calls the counter names and at no other: not in the warm-up, not in render calls;
  growth                       a cell above the threshold inside the margin grows the box by that cell at the next refit;
  demo mode                    fits once, after rebuild_voxels();
  sixty train steps            fit + skip on the procedural scene: the box stays in the outer box and around every occupied cell.
"""
import pytest
import torch

import ray_bounds_ref as B
import scene_fit_ref as F
from test_pdf_sampler_gpu import SIZES
from test_ray_bounds_model_gpu import _draws, _same, bits_equal
from test_voxel_gpu import BMAX, BMIN, _voxel_model

pytestmark = pytest.mark.gpu
G = 16
CUBE = (BMIN,) * 3 + (BMAX,) * 3
VOXEL = dict(coarse_sampler="voxel", grid_nerf=G, voxel_warmup_epoch=0, voxel_beta=0.1)
BLOB = ((5, 6, 5), (10, 9, 10))                             # cells: [-1.3125, 1.3125] x [-0.875, 0.875] x [-1.3125, 1.3125] without a margin


def _run(dev, kw, d, o, seed_draws, vox=None, epoch=0):
    """A fresh model (same parameters every time; its grid set to `vox` when given): one train render with its backward, then one test
    render -> the model and everything the two modes must share."""
    from mc_nerf_amd.model import MC_NeRF_Loss
    m, _, _, _ = _voxel_model(dev, "f32", d.shape[0], **kw)
    if vox is not None:
        m.sigma_voxels.copy_(vox.to(dev))
    g = torch.Generator().manual_seed(seed_draws)
    N, pdf = d.shape[0], m.settings.pdf
    dr = _draws(m, N, g, pdf)
    gt = torch.rand(N, 3, generator=g)
    dd, od = d.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    rgb_c, rgb_f = m.render_rays_train(dd, od, epoch, 1.0, **{k: v.to(dev) for k, v in dr.items()})
    sel = lambda s: None if s is None else (s[0][:int(s[1].item())].clone(), s[1].clone())
    exact = dict(rgb_c=rgb_c.detach().clone(), rgb_f=rgb_f.detach().clone(), fine_list=sel(m.last_selection), coarse_list=sel(m.last_coarse_selection),
                 z_all=None if m.last_z_all is None else m.last_z_all.clone(), span_train=m.last_ray_span,
                 hit_train=None if m.last_ray_hit is None else m.last_ray_hit.clone())
    MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, gt.to(dev)]).backward()
    exact["d_rays"] = (dd.grad.clone(), od.grad.clone())
    exact["d_params"] = tuple(torch.cat([p.grad.reshape(-1) for p in net.parameters()]) for net in (m.nerf_coarse, m.nerf_fine))
    exact["vox"] = m.sigma_voxels.clone() if m.settings.voxel else None
    test = {k: v.to(dev) for k, v in dr.items() if k not in ("jitter", "u")}
    exact["test"] = m.render_rays_test(d.to(dev), o.to(dev), m.nerf_coarse, m.nerf_fine, **test)
    exact["test_list"], exact["test_z_all"], exact["span_test"] = sel(m.last_selection), m.last_z_all, m.last_ray_span
    return m, exact


KEYS = ("rgb_c", "rgb_f", "fine_list", "coarse_list", "z_all", "span_train", "hit_train", "vox", "test", "test_list", "test_z_all", "span_test")


# ------------------------------------------------------------------------------------------- "fixed" and the absent key
@pytest.mark.parametrize("fine", ["threshold", "pdf"])
def test_fixed_is_the_absent_key_and_never_opens_the_library(gpu_device, monkeypatch, fine):
    from mc_nerf_amd import _fit

    def unloadable():
        raise AssertionError("the fit library was opened")
    monkeypatch.setattr(_fit._B, "lib", unloadable)              # the instance's: `_fit.call` is its bound method and calls self.lib()
    monkeypatch.setattr(_fit, "lib", unloadable)
    with pytest.raises(AssertionError, match="the fit library was opened"):     # ... so the patch does bite
        _fit.call("mcnerf_fit_ray_depths", None, None, 0, None, 1.0, 8.0, None, None, 4, None, 0, None, None, None, None, 0)
    d, o = B.model_rays(256)
    kw = dict(fine_sampler=fine, n_importance=SIZES["small"][1], ray_bounds="aabb", ray_bounds_box=B.BOX, ray_bounds_miss="skip", **VOXEL)
    m_a, e_a = _run(gpu_device, kw, d, o, 31)
    m_f, e_f = _run(gpu_device, dict(kw, ray_bounds_fit="fixed", ray_bounds_fit_margin=0, ray_bounds_fit_every=1), d, o, 31)
    assert m_f.settings.ray_bounds_fit == "fixed" and not m_f.settings.fit_box and m_f._scene is None and m_a._scene is None
    assert m_f.last_scene_box is None and m_a.last_scene_box is None
    for key in KEYS:
        _same(e_f[key], e_a[key], key)
    assert 0 < int(e_a["hit_train"].sum()) < 256


# ------------------------------------------------------------------------------------------------ a grid left at sigma_init
@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("miss", ["sample", "skip"])
@pytest.mark.parametrize("fine", ["threshold", "pdf"])
def test_a_grid_at_sigma_init_fits_the_outer_box_and_renders_like_fixed_mode(gpu_device, fine, miss, N):
    """Every cell holds sigma_init = 30 > voxel_thresh = 0: the fitted cell range is the whole grid, clamped to the outer box, which is then
    the box.  Everything of the train render and the test render is the fixed mode's with that box, bit for bit: colours, lists, rows,
    spans, flags, the grid after the update, and the ray gradients.  The parameter gradients cannot be: two runs of the FIXED mode differ
    in them (measured on MI355X, all eight cases: fixed - fixed 0.8e-9 .. 5.1e-9, fit - fixed 1.0e-9 .. 3.5e-9, on tensors whose largest
    entry is 1.3e-3 .. 3.9e-3; ray gradients 0 in both), so the fit mode's are required to lie among the fixed mode's own runs (below)."""
    dev = gpu_device
    d, o = B.model_rays(N)
    kw = dict(fine_sampler=fine, n_importance=SIZES["small"][1], ray_bounds="aabb", ray_bounds_box=B.BOX, ray_bounds_miss=miss, **VOXEL)
    m_x, e_x = _run(dev, kw, d, o, 37)
    m_v, e_v = _run(dev, dict(kw, ray_bounds_fit="voxel"), d, o, 37)
    assert m_v.settings.fit_box and m_v.settings.box == m_x.settings.box and m_v.last_scene_box is m_v.scene_box
    assert m_v.scene_box.tolist() == list(m_x.settings.box) and m_v.scene_cells.tolist() == [0, 0, 0, G - 1, G - 1, G - 1, 1, 0]
    assert m_v.scene_box_status() == 1
    for key in KEYS:
        _same(e_v[key], e_x[key], key)
    # the ray gradients: bit for bit
    _same(e_v["d_rays"], e_x["d_rays"], "d_rays")
    assert all(float(x.abs().max()) > 0 for x in e_x["d_rays"])
    # the parameter gradients.  They leave the kernels through float atomics, whose order changes from run to run, so "the fixed mode's
    # gradients" are a set: seven runs of it stand for that set, and the fit mode's run must lie in it -- no farther (largest entry of the
    # difference) from the nearest of the seven than the two of them that differ most differ from each other.  Were the seven to agree bit
    # for bit this would be equality.  No factor, no tolerance: if the fit run is one more draw from the fixed mode's distribution, its
    # nearest of 7 distances exceeds the largest of the 21 among them with probability 1 / C(28, 7) < 1e-6.
    fixed = [e_x] + [_run(dev, kw, d, o, 37)[1] for _ in range(6)]
    dist = lambda a, b: float((a - b).abs().max())
    for i, a in enumerate(e_v["d_params"]):
        spread = max(dist(fixed[p]["d_params"][i], fixed[q]["d_params"][i]) for p in range(7) for q in range(p))
        near = min(dist(a, f["d_params"][i]) for f in fixed)
        print(f"[{fine} {miss} N={N}] d_params[{i}]: fit to the nearest fixed run {near:.3e}, fixed runs among themselves up to {spread:.3e}, "
              f"max {float(e_x['d_params'][i].abs().max()):.3e}")
        assert near <= spread, (i, near, spread)
        assert float(e_x["d_params"][i].abs().max()) > 0
    assert (e_x["hit_train"] is None) == (miss == "sample") and float(e_x["d_params"][0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------- a known blob
@pytest.mark.parametrize("margin", [0, 2])
@pytest.mark.parametrize("fine, miss", [("threshold", "skip"), ("pdf", "sample")])
def test_a_known_blob_gives_the_restated_box_and_the_fixed_models_render(gpu_device, fine, miss, margin):
    from mc_nerf_amd import ops
    dev, N = gpu_device, 256
    d, o = B.model_rays(N)
    vox = F.blob(G, *BLOB)
    kw = dict(fine_sampler=fine, n_importance=SIZES["small"][1], ray_bounds="aabb", ray_bounds_miss=miss, **VOXEL)
    m_v, e_v = _run(dev, dict(kw, ray_bounds_fit="voxel", ray_bounds_fit_margin=margin), d, o, 41, vox)
    grid = m_v.voxel_grid()
    r_cells, r_box = F.voxel_box_ref(vox, grid.bmin, grid.h, 0.0, margin, CUBE)
    assert r_cells.tolist() == [*BLOB[0], *BLOB[1], 1, 0] and r_box.tolist() == list(F.box_of_cells([v - margin for v in BLOB[0]], [v + margin for v in BLOB[1]], grid.bmin, grid.h))
    assert bits_equal(m_v.last_scene_box, r_box.to(dev)) and torch.equal(m_v.scene_cells.cpu(), r_cells) and m_v.scene_box_status() == 1
    # the span and the flag of the last (test) render, and of the train render, are ops.ray_depths' on the six numbers
    six = tuple(r_box.tolist())
    _, _, span, hit = ops.ray_depths(o.to(dev), d.to(dev), six, m_v.near, m_v.far, None, m_v.z_vals_c, want_hit=True)
    assert bits_equal(m_v.last_ray_span, span) and bits_equal(e_v["span_test"], span)
    assert (m_v.last_ray_hit is None) if miss == "sample" else torch.equal(m_v.last_ray_hit, hit)
    assert (e_v["hit_train"] is None) if miss == "sample" else torch.equal(e_v["hit_train"], hit)
    assert 0 < int(hit.sum()) < N
    # a fixed-box model given those six numbers
    m_x, e_x = _run(dev, dict(kw, ray_bounds_box=six), d, o, 41, vox)
    assert m_x.settings.box == six and not m_x.settings.fit_box
    for key in KEYS:
        _same(e_v[key], e_x[key], key)


# ------------------------------------------------------------------------------------------------------------------ cadence
def test_the_box_changes_at_the_calls_the_counter_names_and_at_no_other(gpu_device):
    dev, N, every, warmup = gpu_device, 64, 3, 2
    d, o = B.model_rays(N)
    kw = dict(ray_bounds="aabb", ray_bounds_fit="voxel", ray_bounds_fit_margin=1, ray_bounds_fit_every=every, **dict(VOXEL, voxel_warmup_epoch=warmup))
    m, _, _, _ = _voxel_model(dev, "f32", N, **kw)
    m.sigma_voxels.copy_(F.blob(G, *BLOB).to(dev))
    grid, dd, od = m.voxel_grid(), d.to(dev), o.to(dev)
    fit_of = lambda vox: F.voxel_box_ref(vox, grid.bmin, grid.h, 0.0, 1, CUBE)[1]
    assert m.last_scene_box is None
    torch.manual_seed(3)
    seen = []
    for call, epoch in enumerate([0, 1, 2, 3, 4, 5, 6, 7, 8]):
        before, vox = m.scene_box.clone(), m.sigma_voxels.cpu().clone()
        if call == 4:                                                           # a far corner cell, by hand, between two refits
            m.sigma_voxels[0, G - 1, 0] = 9.0
            vox = m.sigma_voxels.cpu().clone()
        m.render_rays_train(dd, od, epoch, 1.0)
        refit = epoch >= warmup and (epoch - warmup) % every == 0             # post-warm-up calls 0, 3, 6
        assert m.last_scene_box is m.scene_box
        if refit:
            assert bits_equal(m.scene_box.cpu(), fit_of(vox)), (call, m.scene_box.tolist())
        else:
            assert bits_equal(m.scene_box, before), call
        seen.append(m.scene_box.cpu().clone())
        calls = m._fit_calls
        m.render_rays_test(dd, od, m.nerf_coarse, m.nerf_fine)                  # render calls never refit, and do not count
        assert bits_equal(m.scene_box.cpu(), seen[-1]) and m._fit_calls == calls and m.last_scene_box is m.scene_box
    assert [s.tolist() for s in seen[:2]] == [list(CUBE)] * 2                   # the warm-up: the outer box
    assert seen[2].tolist() != list(CUBE) and bits_equal(seen[3], seen[2]) and bits_equal(seen[4], seen[2])
    assert not bits_equal(seen[5], seen[4]) and float(seen[5][0]) == BMIN and float(seen[5][4]) == BMAX      # the corner cell, at the call the counter names
    assert m._fit_calls == 7 and m.scene_box_status() == 1


# ------------------------------------------------------------------------------------------------------------------- growth
def test_a_cell_inside_the_margin_grows_the_box_by_that_cell(gpu_device):
    dev = gpu_device
    kw = dict(ray_bounds="aabb", ray_bounds_fit="voxel", ray_bounds_fit_margin=2, **VOXEL)
    m, _, _, _ = _voxel_model(dev, "f32", 64, **kw)
    vox = F.blob(G, *BLOB)
    m.sigma_voxels.copy_(vox.to(dev))
    grid = m.voxel_grid()
    box = m.refit_scene_box()
    assert box is m.scene_box and m.scene_cells.tolist() == [*BLOB[0], *BLOB[1], 1, 0]
    first = box.cpu().clone()
    assert first.tolist() == list(F.box_of_cells([v - 2 for v in BLOB[0]], [v + 2 for v in BLOB[1]], grid.bmin, grid.h))
    # one cell beyond the occupied range in +x, inside the margin (so inside the box: a sample there is evaluated) and empty so far
    cell = (BLOB[1][0] + 1, 7, 7)
    centre = [grid.bmin + (c + 0.5) * grid.h for c in cell]
    assert all(first[k] < centre[k] < first[3 + k] for k in range(3)) and float(vox[cell]) < 0
    m.sigma_voxels[cell] = 0.5
    m.refit_scene_box()
    grown = m.scene_box.cpu()
    assert m.scene_cells.tolist() == [*BLOB[0], BLOB[1][0] + 1, *BLOB[1][1:], 1, 0]
    want = first.clone()
    want[3] = torch.tensor(grid.bmin) + torch.tensor(float(BLOB[1][0] + 1 + 2 + 1)) * torch.tensor(grid.h)
    assert bits_equal(grown, want) and float(grown[3]) > float(first[3])         # xmax alone, by one cell
    # with margin 0 the same cell lies outside the box: nothing evaluates it, and the box can only shrink
    m0, _, _, _ = _voxel_model(dev, "f32", 64, **dict(kw, ray_bounds_fit_margin=0))
    m0.sigma_voxels.copy_(vox.to(dev))
    tight = m0.refit_scene_box().cpu()
    assert not float(tight[0]) < centre[0] < float(tight[3])


# ---------------------------------------------------------------------------------------------------------------- demo mode
def test_demo_mode_fits_once_after_rebuild_voxels(gpu_device, tmp_path):
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd.model import NeRF_Model
    dev = gpu_device
    trained, _, _, _ = _voxel_model(dev, "f32", 64, seed=3)
    path = str(tmp_path / "ref_format.ckpt")
    torch.save({"model_nerf": {f"nerf.{k}": v for k, v in trained.state_dict().items()}}, path)
    Sc, _, coarse, fine = SIZES["small"]
    grids = {}
    for thresh in (-1e30, 1e30):                                                # every cell occupied; no cell occupied
        demo = NeRF_Model(S.make_sys_param(dev, mode=1, demo_ckpt=path, samples=Sc, scale=2, batch=64, H=8, W=8, coarse=coarse, fine=fine,
                                           ray_bounds="aabb", ray_bounds_fit="voxel", voxel_thresh=thresh, **VOXEL)).to(dev)
        assert demo._scene is not None and list(demo.state_dict()) == list(trained.state_dict())
        grid = demo.voxel_grid()
        r_cells, r_box = F.voxel_box_ref(demo.sigma_voxels.cpu(), grid.bmin, grid.h, thresh, 2, CUBE)
        assert torch.equal(demo.scene_cells.cpu(), r_cells) and bits_equal(demo.scene_box.cpu(), r_box)
        assert demo.scene_box_status() == (1 if thresh < 0 else 0)
        grids[thresh] = demo.sigma_voxels.clone()
        # a render reads the box and does not refit it
        demo.sigma_voxels.fill_(-1e31 if thresh < 0 else 1e31)
        d, o = B.model_rays(64)
        before = demo.scene_cells.clone()
        demo.render_rays_test(d.to(dev), o.to(dev), demo.nerf_coarse, demo.nerf_fine)
        assert torch.equal(demo.scene_cells, before) and demo.last_scene_box is demo.scene_box and demo._fit_calls == 0
    assert torch.equal(grids[-1e30], grids[1e30])


# -------------------------------------------------------------------------------------------------------- sixty train steps
@pytest.mark.parametrize("N", [64, 256])
def test_sixty_train_steps_in_fit_and_skip_mode(gpu_device, N):
    from mc_nerf_amd import ops, synthetic as S
    from mc_nerf_amd.model import MC_NeRF_Loss, NeRF_Model, RAdam
    dev, H, W, steps, warmup, every = gpu_device, 32, 32, 60, 12, 8
    torch.manual_seed(0)
    pose, K, _ = S.ball_cameras(seed=0, radius=3.0, H=H, W=W)
    pose, K = pose.to(dev), K.to(dev)
    Kinv = torch.linalg.inv(K)
    imgs = S.blob_scene_images(pose, K, H, W)
    Sc, _, coarse, fine = SIZES["small"]
    sp = S.make_sys_param(dev, samples=Sc, scale=2, batch=N, H=H, W=W, coarse=coarse, fine=fine, precision="f32", ray_bounds="aabb",
                          ray_bounds_miss="skip", ray_bounds_fit="voxel", ray_bounds_fit_every=every, **dict(VOXEL, voxel_warmup_epoch=warmup))
    model = NeRF_Model(sp).to(dev)
    opt = RAdam(model.parameters(), lr=2e-3, weight_decay=0.0)
    loss_fn = MC_NeRF_Loss(sp)
    grid = model.voxel_grid()
    outer = torch.tensor(CUBE)
    losses, boxes, refits, hits = [], [], 0, []
    for step in range(steps):
        i = (7 * step) % pose.shape[0]
        pix = torch.randperm(H * W, device=dev)[:N]
        d, o = ops.raygen_fwd(pose[i].contiguous(), Kinv[i].contiguous(), pix, W)
        refit = step >= warmup and (step - warmup) % every == 0
        vox = model.sigma_voxels.cpu().clone() if refit else None
        rgb_c, rgb_f = model.render_rays_train(d, o, step, 1.0)
        loss = loss_fn.get_rgb_loss([rgb_c, rgb_f, imgs[i][pix]])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        box = model.last_scene_box.cpu().clone()
        boxes.append(box)
        hits.append(model.last_ray_hit.sum())
        assert bool((box[:3] >= outer[:3]).all()) and bool((box[3:] <= outer[3:]).all()) and bool((box[:3] < box[3:]).all())
        if refit:
            refits += 1
            r_cells, r_box = F.voxel_box_ref(vox, grid.bmin, grid.h, 0.0, 2, CUBE)
            assert bits_equal(box, r_box) and torch.equal(model.scene_cells.cpu(), r_cells)
            occ = torch.nonzero(vox > 0).to(torch.float32)
            if occ.shape[0]:                                                    # every occupied cell, with its whole extent, lies inside the box
                lo = torch.tensor(grid.bmin) + occ.min(0).values * torch.tensor(grid.h)
                hi = torch.tensor(grid.bmin) + (occ.max(0).values + 1.0) * torch.tensor(grid.h)
                assert bool((box[:3] <= lo).all()) and bool((box[3:] >= torch.fmin(hi, outer[3:])).all())
        elif step > 0:
            assert bits_equal(box, boxes[-2])
    losses = torch.stack(losses).cpu()
    hits = torch.stack(hits).cpu()
    status = model.scene_box_status()
    print(f"[fit + skip, {N} rays x {steps} steps] loss {float(losses[0]):.4f} -> {float(losses[-10:].mean()):.4f}; {refits} refits; final box "
          f"{[round(v, 3) for v in boxes[-1].tolist()]}, cells {model.scene_cells.tolist()}; rays that hit: first {int(hits[0])}, last {int(hits[-1])} of {N}")
    assert bool(torch.isfinite(losses).all()) and refits == 6 and int(opt.skipped_steps()) == 0
    assert status == 1
