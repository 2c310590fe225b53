"""Per-ray sample bounds through the renderer and the models (sys_param key "ray_bounds").  Small nets, at most 512 rays.

  a box that clips nothing   "aabb" with a +-1e3 box against "global", for threshold and pdf, dense and voxel (past the warm-up), the train
                             and the test render: the colours, the lists and counts, last_z_all, the voxel grid and depth / opacity bit
                             for bit; last_ray_span = (near, far) everywhere.  The ray and parameter gradients are float-atomic sums
                             whose order changes from run to run -- two runs of "global" itself do not agree to the bit -- so they are
                             held to the gate of tests/test_pdf_sampler_gpu.py::test_depth_rows_equal_the_grid_call (`_spread_ok`, on
                             the ray gradients and each net's flat gradient as there), and to equality whenever the runs of "global"
                             do agree to the bit;
  a clipping box             on rays of which between 1/2 and 9/10 are clipped and some miss (tests/test_ray_bounds_cpu.py asserts the
                             shares): the samples of a clipped ray lie in the box; the model's renders equal the same kernels driven by
                             hand through `ops` on the rows of ops.ray_depths, bit for bit; colours and every gradient of one train step
                             against the CPU oracle on those rows (f32 and f16x3);
  voxel + aabb               updates from clipped rays touch no cell outside the set the restatement says their samples reach;
  composition                one MC_Model step with mask_weight, dist_weight, depth_weight, cams_per_step = 2, lens_model = "radial"
                             and aabb: finite, and the same twice from the same draws.
"""
import pytest
import torch

import ray_bounds_ref as B
from oracle import mcnerf_oracle as O
from test_pdf_sampler_gpu import E2E_TOL, SIZES, _spread_ok, err
from test_voxel_gpu import BMAX, BMIN, _ball, _list, _voxel_model

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def _draws(m, N, g, pdf):
    Sc = m.samples_c
    dr = dict(jitter=torch.rand(N, 1, generator=g) * (m.far - m.near) / Sc, eps_c=torch.randn(N, Sc, generator=g), eps_sel=torch.randn(N, Sc, generator=g))
    if pdf:
        dr["u"] = torch.rand(N, m.n_importance, generator=g)
    dr["eps_f"] = torch.randn(N, m.settings.samples_pdf if pdf else m.samples_f, generator=g)
    return dr


# ------------------------------------------------------------------------------------------------ a box that clips nothing
def _train_and_render(dev, kw, d, o, seed_draws):
    """A fresh model (same parameters every time): one train render with its backward, then one test render -> what the two modes share."""
    from mc_nerf_amd.model import MC_NeRF_Loss
    m, _, _, _ = _voxel_model(dev, "f32", d.shape[0], **kw)
    if m.settings.voxel:
        m.sigma_voxels.copy_(_ball(m.grid_nerf).to(dev))
    g = torch.Generator().manual_seed(seed_draws)
    N, pdf = d.shape[0], m.settings.pdf
    dr = _draws(m, N, g, pdf)
    gt = torch.rand(N, 3, generator=g)
    dd, od = d.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    rgb_c, rgb_f = m.render_rays_train(dd, od, 0, 1.0, **{k: v.to(dev) for k, v in dr.items()})
    sel = lambda s: None if s is None else (s[0][:int(s[1].item())].clone(), s[1].clone())
    exact = dict(rgb_c=rgb_c.detach().clone(), rgb_f=rgb_f.detach().clone(), fine_list=sel(m.last_selection), coarse_list=sel(m.last_coarse_selection),
                 z_all=None if m.last_z_all is None else m.last_z_all.clone(), span_train=m.last_ray_span)
    MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, gt.to(dev)]).backward()
    # the ray gradients and each net's whole gradient as one flat tensor: the tensors the gate's own test applies it to
    grads = [dd.grad.clone(), od.grad.clone()] + [torch.cat([p.grad.reshape(-1) for p in net.parameters()]) for net in (m.nerf_coarse, m.nerf_fine)]
    exact["vox"] = m.sigma_voxels.clone() if m.settings.voxel else None
    test = {k: v.to(dev) for k, v in dr.items() if k not in ("jitter", "u")}
    exact["test"] = m.render_rays_test(d.to(dev), o.to(dev), m.nerf_coarse, m.nerf_fine, **test)
    exact["test_list"], exact["test_z_all"], exact["span_test"] = sel(m.last_selection), m.last_z_all, m.last_ray_span
    return m, exact, grads


def _same(a, b, name):
    if a is None or b is None:
        assert a is None and b is None, name
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), name
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{name}[{i}]")
    else:
        assert a.shape == b.shape and torch.equal(a, b), name


@pytest.mark.parametrize("coarse", ["dense", "voxel"])
@pytest.mark.parametrize("fine", ["threshold", "pdf"])
def test_a_box_that_clips_nothing_is_global(gpu_device, fine, coarse):
    from mc_nerf_amd import _box
    dev, N = gpu_device, 256
    d, o = B.model_rays(N)
    kw = dict(fine_sampler=fine, n_importance=SIZES["small"][1])
    if coarse == "voxel":
        kw.update(coarse_sampler="voxel", grid_nerf=16, voxel_warmup_epoch=0, voxel_beta=0.1)
    m_g, e_g, g1 = _train_and_render(dev, kw, d, o, 31)
    _, _, g2 = _train_and_render(dev, kw, d, o, 31)
    _, _, g3 = _train_and_render(dev, kw, d, o, 31)
    m_a, e_a, ga = _train_and_render(dev, dict(kw, ray_bounds="aabb", ray_bounds_box=B.NO_CLIP), d, o, 31)
    assert _box.loaded() and m_a.settings.aabb and not m_g.settings.aabb
    assert e_g["span_train"] is None and e_g["span_test"] is None
    near_far = torch.tensor([m_a.near, m_a.far], device=dev).expand(N, 2)
    assert torch.equal(e_a["span_train"], near_far) and torch.equal(e_a["span_test"], near_far)
    for key in ("rgb_c", "rgb_f", "fine_list", "coarse_list", "z_all", "vox", "test", "test_list", "test_z_all"):
        _same(e_a[key], e_g[key], key)
    assert (e_g["fine_list"] is None) == (fine == "pdf") and (e_g["coarse_list"] is None) == (coarse == "dense")
    if coarse == "voxel":
        assert 0 < e_g["coarse_list"][0].shape[0] < N * m_g.samples_c
    for i, (x1, x2, x3, xa) in enumerate(zip(g1, g2, g3, ga)):
        spread = max(float((x1 - x2).abs().max()), float((x1 - x3).abs().max()))
        ok, info = _spread_ok(xa, x1, spread)
        assert ok, (i, info)
        if spread == 0.0:
            assert torch.equal(xa, x1), (i, info)
        assert float(x1.abs().max()) > 0


# --------------------------------------------------------------------------------------------------------- a clipping box
def _by_hand(m, d, o, jit, eps_c, eps_sel, eps_f, u, step_r):
    """The render of `m` from its kernels driven through ops on the rows of ops.ray_depths (dense coarse pass, no cap)."""
    from mc_nerf_amd import ops
    st, dev, prec = m.settings, d.device, m.settings.precision
    N = d.shape[0]
    z_c, z_f, span = ops.ray_depths(o, d, st.box, m.near, m.far, jit, m.z_vals_c, None if st.pdf else m.z_vals_f)
    barf = m.emmbedding_xyz.barf_weights_on(step_r, dev, pad=10)
    nets = []
    for model in (m.nerf_coarse, m.nerf_fine):
        flat = model.flat_params()
        nets.append((model.net, flat, ops.pack_weights(model.net, flat, precision=prec)))
    out_c = torch.empty(N, st.samples_c, 4, device=dev)
    ops.mlp_fwd(*nets[0], o, d, None, None, barf, out_c, precision=prec, z_rows=z_c)
    rgb_c, _, _, w_sel, wmax = ops.composite_fwd(out_c, d, None, None, eps_c, eps_sel, st.white_back, z_rows=z_c)
    if st.pdf:
        rows = ops.sample_pdf(w_sel, None, None, u, z_rows=z_c)
        out_f, lst = torch.empty(*rows.shape, 4, device=dev), None
        ops.mlp_fwd(*nets[1], o, d, None, None, barf, out_f, precision=prec, z_rows=rows)
    else:
        rows = z_f
        idx, count, out_f = ops.select_fine(w_sel, wmax, st.weight_thresh, st.scale, st.sigma_default)
        ops.mlp_fwd(*nets[1], o, d, None, None, barf, out_f, idx=idx, count=count, max_rows=N * st.samples_f, precision=prec, z_rows=rows)
        lst = idx[:int(count.item())]
    rgb_f, depth, opacity, _, _ = ops.composite_fwd(out_f, d, None, None, eps_f, None, st.white_back, want_depth=True, z_rows=rows)
    return dict(rgb_c=rgb_c, rgb_f=rgb_f, depth=depth, opacity=opacity, z_c=z_c, rows=rows, span=span, list=lst)


@pytest.mark.parametrize("fine", ["threshold", "pdf"])
def test_clipped_renders_are_the_kernels_on_the_rows_and_stay_in_the_box(gpu_device, fine):
    dev, N = gpu_device, 256
    d, o = B.model_rays(N)
    m, _, _, _ = _voxel_model(dev, "f32", N, fine_sampler=fine, n_importance=SIZES["small"][1], ray_bounds="aabb", ray_bounds_box=B.BOX)
    assert (m.near, m.far) == (B.NEAR, B.FAR)
    lo, hi, clipped = B.span_ref(o, d, B.BOX, B.NEAR, B.FAR)
    assert 0.5 <= float(clipped.float().mean()) <= 0.9 and int((~clipped).sum()) >= 1
    g = torch.Generator().manual_seed(41)
    dr = {k: v.to(dev) for k, v in _draws(m, N, g, fine == "pdf").items()}
    dd, od = d.to(dev), o.to(dev)
    # ---- the test render: no jitter
    test = {k: v for k, v in dr.items() if k not in ("jitter", "u")}
    u_lin = torch.linspace(0.0, 1.0, m.n_importance, device=dev).expand(N, -1).contiguous() if fine == "pdf" else None
    rgb, depth, opacity = m.render_rays_test(dd, od, m.nerf_coarse, m.nerf_fine, **test)
    h = _by_hand(m, dd, od, None, test["eps_c"], test["eps_sel"], test["eps_f"], u_lin, 1)
    assert bits_equal(rgb, h["rgb_f"]) and bits_equal(depth, h["depth"]) and bits_equal(opacity, h["opacity"])
    assert bits_equal(m.last_ray_span, h["span"]) and bits_equal(h["span"].cpu(), torch.stack([lo, hi], -1))
    if fine == "pdf":
        assert bits_equal(m.last_z_all, h["rows"]) and m.last_selection is None
    else:
        assert torch.equal(_list(m.last_selection), h["list"].cpu().long()) and m.last_z_all is None and 0 < h["list"].shape[0] < N * m.samples_f
    # every sample of a clipped ray lies in the box.  z is within affine_bound of [lo, hi] (tests/ray_bounds_ref.py), and on the axis that
    # binds d_k lo = (min_k - o_k) (1 + 2 u) (the subtraction and the division): 3 u (|o| + |box|) with the slack, plus |d| times the bound
    tol = float(d.abs().max()) * B.affine_bound(B.FAR, 0.0) + 3.0 * U * (float(o.abs().max()) + max(abs(v) for v in B.BOX))
    box_lo, box_hi = torch.tensor(B.BOX[:3]).double(), torch.tensor(B.BOX[3:]).double()
    for rows in (h["z_c"], h["rows"]):
        p = o.double().unsqueeze(1) + d.double().unsqueeze(1) * rows.cpu().double().unsqueeze(2)
        inside = ((p >= box_lo - tol) & (p <= box_hi + tol)).all(-1)
        assert bool(inside[clipped].all()), int((~inside[clipped]).sum())
        assert not bool(inside[~clipped].all())                             # ... which the rays it does not clip do not
    # ---- the train render: the jittered rows reach a (hi - lo) jitter / (far - near) past hi, as today's reach `jitter` past far
    rgb_c, rgb_f = m.render_rays_train(dd, od, 0, 1.0, **dr)
    h = _by_hand(m, dd, od, dr["jitter"].reshape(-1).contiguous(), dr["eps_c"], dr["eps_sel"], dr["eps_f"], dr.get("u"), 1.0)
    assert bits_equal(rgb_c, h["rgb_c"]) and bits_equal(rgb_f, h["rgb_f"]) and bits_equal(m.last_ray_span, h["span"])
    a = ((hi - lo).double() / (B.FAR - B.NEAR)).unsqueeze(1)
    bound = B.affine_bound(B.FAR, (B.FAR - B.NEAR) / m.samples_c)
    for rows in (h["z_c"], h["rows"]):
        z = rows.cpu().double()
        assert bool((z >= lo.double().unsqueeze(1) - bound).all()) and bool((z <= hi.double().unsqueeze(1) + a * dr["jitter"].cpu().double() + bound).all())


def _oracle_on_rows(pc, pf, cfg, d, o, step_r, dr, z_c, z_f, idx_f, gt, permute):
    """The aabb-mode train render composed from the oracle, whose per-pass inference takes explicit z_vals: coarse inference on the
    coarse rows, fine inference on the device's fine list over the fine rows; loss and every gradient (the depths are constants)."""
    pc = {k: v.detach().clone() for k, v in pc.items()}
    pf = {k: v.detach().clone() for k, v in pf.items()}
    undo = (lambda x: x, lambda x: x)
    if permute:
        (pc, uc), (pf, uf) = O.permute_hidden_units(pc, cfg.coarse, 1), O.permute_hidden_units(pf, cfg.fine, 2)
        undo = (uc, uf)
    for p in list(pc.values()) + list(pf.values()):
        p.requires_grad_(True)
    d_, o_ = d.clone().requires_grad_(True), o.clone().requires_grad_(True)
    rgb_c, _, _, _, _ = O.inference(pc, cfg.coarse, cfg, step_r, o_, d_, z_c, dr["eps_c"])
    rgb_f, _, _, _, _ = O.inference(pf, cfg.fine, cfg, step_r, o_, d_, z_f, dr["eps_f"], idx_render=idx_f)
    loss = O.rgb_loss(rgb_c, rgb_f, gt)
    loss.backward()
    grads = {}
    for tag, p_, un in (("c", pc, undo[0]), ("f", pf, undo[1])):
        for k_, v in un({k_: p.grad for k_, p in p_.items()}).items():
            grads[f"{tag}.{k_}"] = v
    return grads, rgb_c.detach(), rgb_f.detach(), float(loss.detach()), d_.grad, o_.grad


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_clipped_train_step_matches_the_oracle_on_its_rows(gpu_device, precision):
    """The tolerances are E2E_TOL of tests/test_pdf_sampler_gpu.py (the gates of tests/test_model_gpu.py::
    test_sh_degree_topology_matches_reference), applied as tests/test_voxel_gpu.py::test_voxel_train_step_matches_the_oracle_on_its_lists
    applies them."""
    from mc_nerf_amd import ops
    from mc_nerf_amd.model import MC_NeRF_Loss
    dev, N = gpu_device, 256
    tol_rgb, tol_loss, tol_ray, tol_par, k_noise, tol_all = E2E_TOL[precision]
    m, cfg, pc, pf = _voxel_model(dev, precision, N, ray_bounds="aabb", ray_bounds_box=B.BOX)
    d, o = B.model_rays(N)
    g = torch.Generator().manual_seed(43)
    dr = _draws(m, N, g, False)
    gt = torch.rand(N, 3, generator=g)
    dd, od = d.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    rgb_c, rgb_f = m.render_rays_train(dd, od, 0, 1.0, **{k: v.to(dev) for k, v in dr.items()})
    idx_f = _list(m.last_selection)
    assert 0 < idx_f.shape[0] < N * m.samples_f
    z_c, z_f, span = ops.ray_depths(od.detach(), dd.detach(), m.settings.box, m.near, m.far, dr["jitter"].reshape(-1).to(dev), m.z_vals_c, m.z_vals_f)
    assert bits_equal(span, m.last_ray_span) and bits_equal(z_c.cpu(), B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, dr["jitter"], O._grids(cfg)[0])[0])
    z_c, z_f = z_c.cpu(), z_f.cpu()
    ref, r_c, r_f, ref_loss, ref_dd, ref_od = _oracle_on_rows(pc, pf, cfg, d, o, 1.0, dr, z_c, z_f, idx_f, gt, permute=False)
    assert err(rgb_c, r_c) < tol_rgb and err(rgb_f, r_f) < tol_rgb, (err(rgb_c, r_c), err(rgb_f, r_f))
    loss = MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, gt.to(dev)])
    assert abs(float(loss.detach()) - ref_loss) < tol_loss
    loss.backward()
    noise_run, _, _, _, nz_dd, nz_od = _oracle_on_rows(pc, pf, cfg, d, o, 1.0, dr, z_c, z_f, idx_f, gt, permute=True)
    e_d, e_o = err(dd.grad, ref_dd) / float(ref_dd.abs().max()), err(od.grad, ref_od) / float(ref_od.abs().max())
    n_d, n_o = err(nz_dd, ref_dd) / float(ref_dd.abs().max()), err(nz_od, ref_od) / float(ref_od.abs().max())
    assert e_d < tol_ray and e_o < tol_ray, (e_d, n_d, e_o, n_o)
    num = den = worst = 0.0
    for tag, net in (("c", m.nerf_coarse), ("f", m.nerf_fine)):
        for k_, p in net.named_parameters():
            r_ = ref[f"{tag}.{k_}"]
            num += float(((p.grad.detach().cpu().double() - r_.double()) ** 2).sum())
            den += float((r_.double() ** 2).sum())
            scale = float(r_.abs().max())
            e = err(p.grad, r_) / max(scale, 1e-30)
            noise = float((noise_run[f"{tag}.{k_}"] - r_).abs().max()) / max(scale, 1e-30)
            worst = max(worst, e)
            if tol_par is not None:
                assert e < max(tol_par, k_noise * noise), (tag, k_, e, noise)
    e_all = (num / den) ** 0.5
    assert e_all < tol_all, e_all
    print(f"[aabb step {precision}] rgb {max(err(rgb_c, r_c), err(rgb_f, r_f)):.1e}, d_rays_d {e_d:.1e} / d_rays_o {e_o:.1e} (oracle reorder noise "
          f"{n_d:.1e} / {n_o:.1e}), worst parameter gradient {worst:.1e} of its tensor's max, whole gradient {e_all:.1e}")


# ------------------------------------------------------------------------------------------------------------- voxel + aabb
def test_voxel_updates_from_clipped_rays_stay_in_the_cells_their_samples_reach(gpu_device):
    dev, G = gpu_device, 16
    d, o = B.model_rays(512)
    keep = B.span_ref(o, d, B.BOX, B.NEAR, B.FAR)[2]
    d, o = d[keep].contiguous(), o[keep].contiguous()
    N = d.shape[0]
    assert 256 <= N <= 512
    touched = {}
    for mode in ("aabb", "global"):
        m, cfg, _, _ = _voxel_model(dev, "f32", N, coarse_sampler="voxel", grid_nerf=G, voxel_warmup_epoch=5, voxel_beta=0.5,
                                    ray_bounds=mode, ray_bounds_box=B.BOX)
        v0 = m.sigma_voxels.clone()
        g = torch.Generator().manual_seed(47)
        dr = _draws(m, N, g, False)
        m.render_rays_train(d.to(dev), o.to(dev), 0, 1.0, **{k: v.to(dev) for k, v in dr.items()})      # (the warm-up: dense, then the update)
        assert m.last_coarse_selection is None and int(m.voxel_grid().scratch.count_nonzero()) == 0
        touched[mode] = (m.sigma_voxels != v0).reshape(-1).cpu()
    rows = B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, dr["jitter"], O._grids(cfg)[0])[0]
    reach = torch.zeros(G ** 3, dtype=torch.bool)
    reach[B.cells_rows(o, d, rows, G, BMIN, BMAX).reshape(-1)] = True
    assert int(touched["aabb"].sum()) > 0 and not bool((touched["aabb"] & ~reach).any())
    # the box's samples reach only the cells the box meets, one sample spacing of slack included
    c = torch.stack(torch.meshgrid(*[torch.arange(G)] * 3, indexing="ij"), -1).reshape(-1, 3).float()
    size = (BMAX - BMIN) / G
    slack = (B.FAR - B.NEAR) / m.samples_c
    c_lo, c_hi = BMIN + c * size, BMIN + (c + 1) * size
    meets = ((c_hi >= torch.tensor(B.BOX[:3]) - slack) & (c_lo <= torch.tensor(B.BOX[3:]) + slack)).all(-1)
    assert not bool((reach & ~meets).any())
    assert bool((touched["global"] & ~meets).any())                        # ... which today's samples of the same rays do not


# --------------------------------------------------------------------------------------------------------------- composition
def test_one_step_with_every_option_on(gpu_device):
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
                              ray_bounds="aabb", ray_bounds_box=B.BOX)
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
        span = model.nerf.last_ray_span
        assert {"rgb", "mask", "dist", "depth"} <= set(loss_dict) and bool(torch.isfinite(loss))
        assert span.shape == (n, 2) and bool((span[:, 1] - span[:, 0] < B.FAR - B.NEAR).any())
        grads = [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(x).all()) for x in grads) and any(float(x.abs().max()) > 0 for x in grads)
        runs.append((loss.detach().clone(), loss_dict["rgb"][0].detach().clone(), loss_dict["rgb"][1].detach().clone(), span.clone(), grads))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for x, y in zip(a[4], b[4]):                            # float-atomic sums: equal to 1e-5 of the tensor's max
        assert float((x - y).abs().max()) <= 1e-5 * float(x.abs().max()) + 1e-12
