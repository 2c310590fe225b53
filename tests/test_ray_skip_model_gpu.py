"""Skipping the rays that miss the scene box through the renderer and the models (sys_param key "ray_bounds_miss").  Small
nets, 256 rays of which 165 hit tests/ray_bounds_ref.py's BOX and 91 miss it (tests/test_ray_skip_cpu.py asserts the counts).

  "sample" and the absent key  the same bits as aabb mode without the key, with the hit library made unloadable; last_ray_hit is None;
  the kernels by hand          the "skip" train and test renders equal the same kernels driven through `ops`, bit for bit, in threshold and
                               pdf, dense and voxel mode (warm-up and pruned): last_ray_hit is the restatement's flag, the dense coarse
                               count is Sc * #hit, no list names a missed ray, a missed ray renders white and its ray gradients are
                               exact zeros;
  the voxel grid               a "skip" train call changes only cells that hit rays' samples reach;
  against "sample"             the hit rays of a test render (pdf mode) and of an only_coarse render, all five precisions, within
                               E2E_TOL[precision][0]: the bound tests/test_voxel_gpu.py::test_a_fresh_grid_lists_every_pair_and_renders_
                               like_dense_mode puts on the same listed-against-dense comparison;
  the oracle step              one train step against the CPU oracle on the device's rows and lists, f32 and f16x3, by the gates of
                               tests/test_ray_bounds_model_gpu.py::test_clipped_train_step_matches_the_oracle_on_its_rows;
  every ray missing            a box far from the cameras: the step and the render finish, every colour is the prefill's composite, every
                               parameter and ray gradient is exactly zero;
  composition                  one MC_Model step with every option on, plus "skip".
"""
import pytest
import torch

import ray_bounds_ref as B
import ray_skip_ref as R
from oracle import mcnerf_oracle as O
from test_pdf_sampler_gpu import E2E_TOL, MODES, SIZES, err
from test_ray_bounds_model_gpu import _draws, _same, _train_and_render, bits_equal
from test_voxel_gpu import BMAX, BMIN, _ball, _list, _voxel_model

pytestmark = pytest.mark.gpu
N_RAYS = 256
FAR_BOX = (50.0, 50.0, 50.0, 51.0, 51.0, 51.0)               # no ray of cameras at radius 4 reaches it within far = 8
SKIP = dict(ray_bounds="aabb", ray_bounds_box=B.BOX, ray_bounds_miss="skip")


def _hit():
    d, o = B.model_rays(N_RAYS)
    hit = R.hit_ref(o, d, B.BOX, B.NEAR, B.FAR)
    assert (int(hit.sum()), int((hit == 0).sum())) == (165, 91)
    return d, o, hit


# ------------------------------------------------------------------------------------------- "sample" and the absent key
@pytest.mark.parametrize("fine", ["threshold", "pdf"])
def test_sample_is_the_absent_key_and_never_opens_the_library(gpu_device, monkeypatch, fine):
    from mc_nerf_amd import _hit as hit_lib
    dev = gpu_device

    def unloadable():
        raise AssertionError("the hit library was opened")
    monkeypatch.setattr(hit_lib, "lib", unloadable)
    d, o, _ = _hit()
    kw = dict(fine_sampler=fine, n_importance=SIZES["small"][1], ray_bounds="aabb", ray_bounds_box=B.BOX)
    m_a, e_a, _ = _train_and_render(dev, kw, d, o, 31)
    m_s, e_s, _ = _train_and_render(dev, dict(kw, ray_bounds_miss="sample"), d, o, 31)
    assert m_s.settings.ray_bounds_miss == "sample" and m_a.last_ray_hit is None and m_s.last_ray_hit is None
    for key in ("rgb_c", "rgb_f", "fine_list", "coarse_list", "z_all", "span_train", "test", "test_list", "test_z_all", "span_test"):
        _same(e_s[key], e_a[key], key)
    assert e_a["coarse_list"] is None and (e_a["fine_list"] is None) == (fine == "pdf")     # the lists of aabb mode are what they were


# ------------------------------------------------------------------------------------------------- against the kernels by hand
def _by_hand(m, grid, d, o, jit, eps_c, eps_sel, eps_f, u, step_r, prune, update):
    """The "skip" render of `m` from its kernels driven through ops: the flags of ops.ray_depths, both passes listed behind them."""
    from mc_nerf_amd import ops
    st, dev, prec = m.settings, d.device, m.settings.precision
    N, Sc = d.shape[0], m.settings.samples_c
    z_c, z_f, span, hit = ops.ray_depths(o, d, st.box, m.near, m.far, jit, m.z_vals_c, None if st.pdf else m.z_vals_f, want_hit=True)
    barf = m.emmbedding_xyz.barf_weights_on(step_r, dev, pad=10)
    nets = []
    for model in (m.nerf_coarse, m.nerf_fine):
        flat = model.flat_params()
        nets.append((model.net, flat, ops.pack_weights(model.net, flat, precision=prec)))
    if prune:
        idx_c, count_c, out_c = ops.voxel_select(grid, st.voxel_thresh, o, d, None, None, st.sigma_default, z_rows=z_c, hit=hit)
    else:
        idx_c, count_c, out_c = ops.list_rays(hit, Sc, st.sigma_default)
    ops.mlp_fwd(*nets[0], o, d, None, None, barf, out_c, idx=idx_c, count=count_c, max_rows=N * Sc, precision=prec, z_rows=z_c)
    rgb_c, _, _, w_sel, wmax = ops.composite_fwd(out_c, d, None, None, eps_c, eps_sel, st.white_back, z_rows=z_c)
    if update:
        ops.voxel_update(grid, st.voxel_beta, o, d, None, None, out_c, idx_c, count_c, N * Sc, z_rows=z_c)
    if st.pdf:
        rows = ops.sample_pdf(w_sel, None, None, u, z_rows=z_c)
        idx_f, count_f, out_f = ops.list_rays(hit, rows.shape[1], st.sigma_default)
    else:
        rows = z_f
        idx_f, count_f, out_f = ops.select_fine(w_sel, wmax, st.weight_thresh, st.scale, st.sigma_default, hit=hit)
    ops.mlp_fwd(*nets[1], o, d, None, None, barf, out_f, idx=idx_f, count=count_f, max_rows=N * rows.shape[1], precision=prec, z_rows=rows)
    rgb_f, depth, opacity, _, _ = ops.composite_fwd(out_f, d, None, None, eps_f, None, st.white_back, want_depth=True, z_rows=rows)
    return dict(rgb_c=rgb_c, rgb_f=rgb_f, depth=depth, opacity=opacity, rows=rows, span=span, hit=hit, out_c=out_c, out_f=out_f,
                coarse_list=idx_c[:int(count_c.item())].cpu().long(), fine_list=idx_f[:int(count_f.item())].cpu().long())


def _copy_of(m, dev):
    from mc_nerf_amd import ops
    grid = ops.VoxelGrid(m.grid_nerf, m.boader_min, m.boader_max, m.sigma_init, dev)
    grid.vox.copy_(m.sigma_voxels)
    return grid


@pytest.mark.parametrize("coarse", ["dense", "warm-up", "pruned"])
@pytest.mark.parametrize("fine", ["threshold", "pdf"])
def test_skip_renders_are_the_kernels_behind_the_flag(gpu_device, fine, coarse):
    from mc_nerf_amd.model import MC_NeRF_Loss
    dev, N = gpu_device, N_RAYS
    d, o, hit = _hit()
    kw = dict(fine_sampler=fine, n_importance=SIZES["small"][1], **SKIP)
    if coarse != "dense":
        kw.update(coarse_sampler="voxel", grid_nerf=16, voxel_beta=0.5, voxel_warmup_epoch=5 if coarse == "warm-up" else 0)
    m, _, _, _ = _voxel_model(dev, "f32", N, **kw)
    st, voxel = m.settings, coarse != "dense"
    assert st.skip_misses and (m.near, m.far) == (B.NEAR, B.FAR) and m.last_ray_hit is None
    if voxel:
        m.sigma_voxels.copy_(_ball(m.grid_nerf).to(dev))
    Sc, missed = st.samples_c, hit == 0
    g = torch.Generator().manual_seed(41)
    dr = {k: v.to(dev) for k, v in _draws(m, N, g, fine == "pdf").items()}
    gt = torch.rand(N, 3, generator=g).to(dev)

    def check(h, train):
        assert torch.equal(m.last_ray_hit.cpu(), hit) and torch.equal(h["hit"].cpu(), hit) and m.last_ray_hit.dtype == torch.int32
        assert torch.equal(_list(m.last_coarse_selection), h["coarse_list"]) and torch.equal(_list(m.last_selection), h["fine_list"])
        assert bits_equal(m.last_ray_span, h["span"])
        if fine == "pdf":
            assert bits_equal(m.last_z_all, h["rows"]) and torch.equal(h["fine_list"], R.list_rays_ref(hit, st.samples_pdf, st.sigma_default)[0])
        else:
            assert m.last_z_all is None and 0 < h["fine_list"].shape[0] < int(hit.sum()) * st.samples_f
        if coarse == "pruned" or (coarse == "warm-up" and not train):           # rendering always queries the grid
            assert 0 < h["coarse_list"].shape[0] < Sc * int(hit.sum())
        else:
            assert int(m.last_coarse_selection[1].item()) == Sc * int(hit.sum())
            assert torch.equal(h["coarse_list"], R.list_rays_ref(hit, Sc, st.sigma_default)[0])
        for lst in (h["coarse_list"], h["fine_list"]):                          # no list names a missed ray
            assert not bool(missed[lst[:, 0]].any())
        # a missed ray's rows are the prefill, in both passes
        for out in (h["out_c"], h["out_f"]):
            assert bits_equal(out.cpu()[missed], R.prefill_ref(N, out.shape[1], st.sigma_default)[missed])

    # ---- the test render: no jitter
    test = {k: v for k, v in dr.items() if k not in ("jitter", "u")}
    u_lin = torch.linspace(0.0, 1.0, m.n_importance, device=dev).expand(N, -1).contiguous() if fine == "pdf" else None
    dd, od = d.to(dev), o.to(dev)
    rgb, depth, opacity = m.render_rays_test(dd, od, m.nerf_coarse, m.nerf_fine, **test)
    h = _by_hand(m, m.voxel_grid() if voxel else None, dd, od, None, test["eps_c"], test["eps_sel"], test["eps_f"], u_lin, 1, prune=voxel, update=False)
    assert bits_equal(rgb, h["rgb_f"]) and bits_equal(depth, h["depth"]) and bits_equal(opacity, h["opacity"])
    check(h, train=False)
    assert float((rgb.cpu()[missed] - 1.0).abs().max()) <= 1e-6 and float((opacity.cpu()[missed] - 1.0).abs().max()) <= 1e-6
    # ---- the train render and its backward
    grid = _copy_of(m, dev) if voxel else None
    dd, od = d.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    rgb_c, rgb_f = m.render_rays_train(dd, od, 0, 1.0, **dr)
    h = _by_hand(m, grid, dd.detach(), od.detach(), dr["jitter"].reshape(-1).contiguous(), dr["eps_c"], dr["eps_sel"], dr["eps_f"], dr.get("u"), 1.0,
                 prune=coarse == "pruned", update=voxel)
    assert bits_equal(rgb_c, h["rgb_c"]) and bits_equal(rgb_f, h["rgb_f"])
    check(h, train=True)
    if voxel:
        assert bits_equal(m.sigma_voxels, grid.vox) and int(m.voxel_grid().scratch.count_nonzero()) == 0
    for rgb in (rgb_c, rgb_f):
        assert float((rgb.detach().cpu()[missed] - 1.0).abs().max()) <= 1e-6
    MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, gt]).backward()
    for grad in (dd.grad.cpu(), od.grad.cpu()):
        assert bool((grad[missed] == 0).all()) and float(grad[~missed].abs().max()) > 0
    assert all(float(p.grad.abs().max()) > 0 for p in list(m.nerf_coarse.parameters())[:1] + list(m.nerf_fine.parameters())[:1])


# ------------------------------------------------------------------------------------------------------------- the voxel grid
def test_missed_rays_do_not_touch_the_voxel_grid(gpu_device):
    dev, N, G = gpu_device, N_RAYS, 16
    d, o, hit = _hit()
    touched = {}
    for miss in ("skip", "sample"):
        m, cfg, _, _ = _voxel_model(dev, "f32", N, coarse_sampler="voxel", grid_nerf=G, voxel_warmup_epoch=5, voxel_beta=0.5,
                                    ray_bounds="aabb", ray_bounds_box=B.BOX, ray_bounds_miss=miss)
        v0 = m.sigma_voxels.clone()
        g = torch.Generator().manual_seed(47)
        dr = _draws(m, N, g, False)
        m.render_rays_train(d.to(dev), o.to(dev), 0, 1.0, **{k: v.to(dev) for k, v in dr.items()})      # (the warm-up: every listed sample updates)
        assert int(m.voxel_grid().scratch.count_nonzero()) == 0 and (m.last_coarse_selection is None) == (miss == "sample")
        touched[miss] = (m.sigma_voxels != v0).reshape(-1).cpu()
    rows = B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, dr["jitter"], O._grids(cfg)[0])[0]
    cells = B.cells_rows(o, d, rows, G, BMIN, BMAX)
    reach = torch.zeros(G ** 3, dtype=torch.bool)
    reach[cells[hit != 0].reshape(-1)] = True
    assert int(touched["skip"].sum()) > 0 and not bool((touched["skip"] & ~reach).any())
    assert bool((touched["sample"] & ~reach).any())                        # ... which the missed rays' samples do when they are evaluated


# ----------------------------------------------------------------------------------------------------------- against "sample"
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("mode", ["only_coarse", "pdf"])
def test_skip_renders_the_hit_rays_like_sample(gpu_device, mode, precision):
    dev, N = gpu_device, N_RAYS
    d, o, hit = _hit()
    tol = E2E_TOL[precision][0]
    kw = dict(fine_sampler="pdf" if mode == "pdf" else "threshold", n_importance=SIZES["small"][1], ray_bounds="aabb", ray_bounds_box=B.BOX)
    outs = {}
    for miss in ("sample", "skip"):
        m, _, _, _ = _voxel_model(dev, precision, N, ray_bounds_miss=miss, **kw)
        g = torch.Generator().manual_seed(53)
        dr = {k: v.to(dev) for k, v in _draws(m, N, g, mode == "pdf").items()}
        with torch.no_grad():
            if mode == "only_coarse":
                rgb, _, depth = m.render_rays_train(d.to(dev), o.to(dev), 0, 1.0, True, jitter=dr["jitter"], eps_c=dr["eps_c"])
                outs[miss] = (rgb, depth)
            else:
                outs[miss] = m.render_rays_test(d.to(dev), o.to(dev), m.nerf_coarse, m.nerf_fine, eps_c=dr["eps_c"], eps_sel=dr["eps_sel"], eps_f=dr["eps_f"])
        assert (m.last_ray_hit is None) == (miss == "sample")
    keep = hit != 0
    errs = [err(a.cpu()[keep], b.cpu()[keep]) for a, b in zip(outs["skip"], outs["sample"])]
    print(f"[skip against sample, {mode} {precision}] hit rays: " + ", ".join(f"{e:.1e}" for e in errs) + f" (gate {tol:.0e})")
    assert all(e < tol for e in errs), errs
    assert float((outs["skip"][0].cpu()[~keep] - 1.0).abs().max()) <= 1e-6
    assert float((outs["sample"][0].cpu()[~keep] - 1.0).abs().max()) > 1e-6        # ... which the evaluated misses are not


# ------------------------------------------------------------------------------------------------------------- the oracle step
def _oracle_on_lists(pc, pf, cfg, d, o, step_r, dr, z_c, z_f, idx_c, idx_f, gt, permute):
    """tests/test_ray_bounds_model_gpu.py::_oracle_on_rows with the coarse inference on the device's coarse list too."""
    pc = {k: v.detach().clone() for k, v in pc.items()}
    pf = {k: v.detach().clone() for k, v in pf.items()}
    undo = (lambda x: x, lambda x: x)
    if permute:
        (pc, uc), (pf, uf) = O.permute_hidden_units(pc, cfg.coarse, 1), O.permute_hidden_units(pf, cfg.fine, 2)
        undo = (uc, uf)
    for p in list(pc.values()) + list(pf.values()):
        p.requires_grad_(True)
    d_, o_ = d.clone().requires_grad_(True), o.clone().requires_grad_(True)
    rgb_c, _, _, _, _ = O.inference(pc, cfg.coarse, cfg, step_r, o_, d_, z_c, dr["eps_c"], idx_render=idx_c)
    rgb_f, _, _, _, _ = O.inference(pf, cfg.fine, cfg, step_r, o_, d_, z_f, dr["eps_f"], idx_render=idx_f)
    loss = O.rgb_loss(rgb_c, rgb_f, gt)
    loss.backward()
    grads = {}
    for tag, p_, un in (("c", pc, undo[0]), ("f", pf, undo[1])):
        for k_, v in un({k_: p.grad for k_, p in p_.items()}).items():
            grads[f"{tag}.{k_}"] = v
    return grads, rgb_c.detach(), rgb_f.detach(), float(loss.detach()), d_.grad, o_.grad


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_skip_train_step_matches_the_oracle_on_its_lists(gpu_device, precision):
    """The tolerances are E2E_TOL, applied exactly as tests/test_ray_bounds_model_gpu.py::test_clipped_train_step_matches_the_oracle_on_
    its_rows applies them.  Measured on MI355X: f32 rgb 2.4e-7, ray gradients 3.1e-7 / 4.0e-7, whole gradient 8.1e-7; f16x3 rgb 2.4e-7,
    ray gradients 2.8e-5 / 3.0e-5, whole gradient 3.9e-6."""
    from mc_nerf_amd import ops
    from mc_nerf_amd.model import MC_NeRF_Loss
    dev, N = gpu_device, N_RAYS
    tol_rgb, tol_loss, tol_ray, tol_par, k_noise, tol_all = E2E_TOL[precision]
    m, cfg, pc, pf = _voxel_model(dev, precision, N, **SKIP)
    d, o, hit = _hit()
    missed = hit == 0
    g = torch.Generator().manual_seed(43)
    dr = _draws(m, N, g, False)
    gt = torch.rand(N, 3, generator=g)
    dd, od = d.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    rgb_c, rgb_f = m.render_rays_train(dd, od, 0, 1.0, **{k: v.to(dev) for k, v in dr.items()})
    idx_c, idx_f = _list(m.last_coarse_selection), _list(m.last_selection)
    assert torch.equal(idx_c, R.list_rays_ref(hit, m.samples_c, m.settings.sigma_default)[0]) and 0 < idx_f.shape[0] < int(hit.sum()) * m.samples_f
    z_c, z_f, span = ops.ray_depths(od.detach(), dd.detach(), m.settings.box, m.near, m.far, dr["jitter"].reshape(-1).to(dev), m.z_vals_c, m.z_vals_f)
    assert bits_equal(span, m.last_ray_span) and torch.equal(m.last_ray_hit.cpu(), hit)
    z_c, z_f = z_c.cpu(), z_f.cpu()
    ref, r_c, r_f, ref_loss, ref_dd, ref_od = _oracle_on_lists(pc, pf, cfg, d, o, 1.0, dr, z_c, z_f, idx_c, idx_f, gt, permute=False)
    e_rgb = max(err(rgb_c, r_c), err(rgb_f, r_f))
    assert err(rgb_c, r_c) < tol_rgb and err(rgb_f, r_f) < tol_rgb, (err(rgb_c, r_c), err(rgb_f, r_f))
    # the oracle on a missed ray: white within the train noise's 6e-8
    assert float((r_c[missed] - 1.0).abs().max()) <= 6e-8 and float((r_f[missed] - 1.0).abs().max()) <= 6e-8
    loss = MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, gt.to(dev)])
    assert abs(float(loss.detach()) - ref_loss) < tol_loss
    loss.backward()
    assert bool((dd.grad.cpu()[missed] == 0).all()) and bool((od.grad.cpu()[missed] == 0).all())
    noise_run, _, _, _, nz_dd, nz_od = _oracle_on_lists(pc, pf, cfg, d, o, 1.0, dr, z_c, z_f, idx_c, idx_f, gt, permute=True)
    e_d, e_o = err(dd.grad, ref_dd) / float(ref_dd.abs().max()), err(od.grad, ref_od) / float(ref_od.abs().max())
    n_d, n_o = err(nz_dd, ref_dd) / float(ref_dd.abs().max()), err(nz_od, ref_od) / float(ref_od.abs().max())
    num = den = worst = 0.0
    fails = []
    for tag, net in (("c", m.nerf_coarse), ("f", m.nerf_fine)):
        for k_, p in net.named_parameters():
            r_ = ref[f"{tag}.{k_}"]
            num += float(((p.grad.detach().cpu().double() - r_.double()) ** 2).sum())
            den += float((r_.double() ** 2).sum())
            scale = float(r_.abs().max())
            e = err(p.grad, r_) / max(scale, 1e-30)
            noise = float((noise_run[f"{tag}.{k_}"] - r_).abs().max()) / max(scale, 1e-30)
            worst = max(worst, e)
            if tol_par is not None and not e < max(tol_par, k_noise * noise):
                fails.append((tag, k_, e, noise))
    e_all = (num / den) ** 0.5
    print(f"[skip step {precision}] rgb {e_rgb:.1e}, loss {abs(float(loss.detach()) - ref_loss):.1e}, d_rays_d {e_d:.1e} / d_rays_o {e_o:.1e} (oracle "
          f"reorder noise {n_d:.1e} / {n_o:.1e}), worst parameter gradient {worst:.1e} of its tensor's max, whole gradient {e_all:.1e}")
    assert e_d < tol_ray and e_o < tol_ray, (e_d, n_d, e_o, n_o)
    assert not fails, fails
    assert e_all < tol_all, e_all


# ------------------------------------------------------------------------------------------------------------ every ray missing
@pytest.mark.parametrize("fine, coarse", [("threshold", "dense"), ("pdf", "voxel")])
def test_a_box_that_every_ray_misses(gpu_device, fine, coarse):
    from mc_nerf_amd.model import MC_NeRF_Loss
    dev, N = gpu_device, N_RAYS
    d, o, _ = _hit()
    assert int(R.hit_ref(o, d, FAR_BOX, B.NEAR, B.FAR).sum()) == 0
    kw = dict(fine_sampler=fine, n_importance=SIZES["small"][1], ray_bounds="aabb", ray_bounds_box=FAR_BOX, ray_bounds_miss="skip")
    if coarse == "voxel":
        kw.update(coarse_sampler="voxel", grid_nerf=16, voxel_warmup_epoch=0)
    m, _, _, _ = _voxel_model(dev, "f32", N, **kw)
    v0 = m.sigma_voxels.clone() if coarse == "voxel" else None
    g = torch.Generator().manual_seed(59)
    dr = {k: v.to(dev) for k, v in _draws(m, N, g, fine == "pdf").items()}
    dd, od = d.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    rgb_c, rgb_f = m.render_rays_train(dd, od, 0, 1.0, **dr)
    assert int(m.last_ray_hit.sum()) == 0 and int(m.last_coarse_selection[1].item()) == 0 and int(m.last_selection[1].item()) == 0
    MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, torch.rand(N, 3, generator=g).to(dev)]).backward()
    torch.cuda.synchronize()
    for rgb in (rgb_c, rgb_f):                                              # the prefill's composite: white within the train noise
        assert float((rgb.detach() - 1.0).abs().max()) <= 1e-6
    assert bool((dd.grad == 0).all()) and bool((od.grad == 0).all())
    for p in list(m.nerf_coarse.parameters()) + list(m.nerf_fine.parameters()):
        assert p.grad is None or bool((p.grad == 0).all())
    if coarse == "voxel":
        assert torch.equal(m.sigma_voxels, v0)
    test = {k: v for k, v in dr.items() if k not in ("jitter", "u")}
    rgb, depth, opacity = m.render_rays_test(d.to(dev), o.to(dev), m.nerf_coarse, m.nerf_fine, **test)
    torch.cuda.synchronize()
    assert float((rgb - 1.0).abs().max()) <= 1e-6 and float((opacity - 1.0).abs().max()) <= 1e-6
    last = m.last_z_all[:, -1:] if fine == "pdf" else (m.z_vals_f[-1] * torch.ones(N, 1, device=dev))
    assert float((depth - last).abs().max()) <= 1e-5 * B.FAR              # the row's last depth (a missed ray's rows are [near, far]'s)


# --------------------------------------------------------------------------------------------------------------- composition
def test_one_step_with_every_option_on_and_skip(gpu_device):
    from mc_nerf_amd import ops, synthetic as S
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss
    dev, K, H, W, n = gpu_device, 2, 32, 32, 256
    STAGE = "GLOBAL_OPTIM_EPOCH"
    seg = ops.ray_segments(n, K)
    g = torch.Generator().manual_seed(21)
    pix = torch.cat([torch.randperm(H * W, generator=g)[:b - a] for a, b in zip(seg, seg[1:])]).to(dev)
    runs = []
    for _ in range(2):
        sp = S.make_sys_param(dev, samples=32, scale=2, batch=n, H=H, W=W, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision="f32",
                              mask_weight=0.3, dist_weight=0.01, depth_weight=0.5, cams_per_step=K, lens_model="radial",
                              ray_bounds="aabb", ray_bounds_box=B.BOX, ray_bounds_miss="skip")
        torch.manual_seed(3)
        model = MC_Model(sp).to(dev)
        S.init_cameras_near_gt(model)
        gi = torch.Generator().manual_seed(5)
        u8 = torch.randint(0, 256, (model.train_numb, H * W, 4), dtype=torch.uint8, generator=gi)
        depth = torch.rand(model.train_numb, H * W, generator=gi) * 4.0 + 1.5
        images = DeviceImageSet(u8.contiguous().to(dev), H, W, depth=depth.to(dev).contiguous())
        wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
        model.sample_pixels_multi = lambda npix, seg_start: pix
        torch.manual_seed(17)                               # the renderer's draws
        loss_dict, *_ = model((images, torch.tensor([5, 0]), wpts, pts, wpts, pts), 20, STAGE, 0.5)
        loss = MC_NeRF_Loss(sp)(loss_dict, STAGE)
        loss.backward()
        hit, span = model.nerf.last_ray_hit, model.nerf.last_ray_span
        assert {"rgb", "mask", "dist", "depth"} <= set(loss_dict) and bool(torch.isfinite(loss))
        assert hit.shape == (n,) and hit.dtype == torch.int32 and 0 < int(hit.sum()) < n
        assert bool((span[hit == 0] == torch.tensor([B.NEAR, B.FAR], device=dev)).all())
        for sel in (model.nerf.last_coarse_selection, model.nerf.last_selection):
            assert not bool((hit == 0)[_list(sel)[:, 0].to(dev)].any())
        grads = [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(x).all()) for x in grads) and any(float(x.abs().max()) > 0 for x in grads)
        runs.append((loss.detach().clone(), loss_dict["rgb"][0].detach().clone(), loss_dict["rgb"][1].detach().clone(), hit.clone(), grads))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for x, y in zip(a[4], b[4]):                            # float-atomic sums: equal to 1e-5 of the tensor's max
        assert float((x - y).abs().max()) <= 1e-5 * float(x.abs().max()) + 1e-12
