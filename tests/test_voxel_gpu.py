"""The voxel sigma cache (`coarse_sampler = "voxel"`) on the GPU: the select, update and point kernels against their torch restatement
(tests/voxel_ref.py) with torch.equal, `rebuild_voxels` against the oracle's net, a train step and a render against the oracle run on
the device's own coarse and fine lists, the warm-up and the fresh grid against dense mode, the default path untouched by the keys, and a
convergence run."""
import pytest
import torch

import voxel_ref as V
from oracle import mcnerf_oracle as O
from test_pdf_sampler_gpu import E2E_TOL, MODES, SIZES, _rays, _spread_ok, err

pytestmark = pytest.mark.gpu
BMIN, BMAX, SIGMA_INIT, SIGMA_DEFAULT = -3.5, 3.5, 30.0, -20.0
N_K = 257                   # rays of the kernel tests: not a multiple of a wavefront, of the four rays of a workgroup, or of 256


def _zgrid(Sc):
    return torch.linspace(1.0, 8.0, Sc)


def _jitter(N, Sc, g):
    return torch.rand(N, generator=g) * 7.0 / Sc


def _grid_of(kind, G, g):
    if kind == "init":
        return torch.full((G, G, G), SIGMA_INIT)
    if kind == "negative":
        return torch.full((G, G, G), -1.0)
    if kind == "random":
        return torch.rand(G, G, G, generator=g) * 2.0 - 1.0
    raise ValueError(kind)


def _device_grid(vox, dev):
    from mc_nerf_amd import ops
    grid = ops.VoxelGrid(vox.shape[0], BMIN, BMAX, SIGMA_INIT, dev)
    grid.vox.copy_(vox.to(dev))
    return grid


def _ball(G):
    """+5 inside the ball of radius 2 around the origin, -5 outside (by cell centre)."""
    c = V.centres(G, BMIN, BMAX)
    return torch.where(c.norm(dim=-1) < 2.0, torch.tensor(5.0), torch.tensor(-5.0))


# ---------------------------------------------------------------------------------------------------------------- 1. select
@pytest.mark.parametrize("jittered", [True, False])
@pytest.mark.parametrize("kind", ["init", "negative", "random", "one"])
@pytest.mark.parametrize("G", [4, 33])
@pytest.mark.parametrize("Sc", [32, 64])
def test_select_kernel_equals_the_restatement(gpu_device, Sc, G, kind, jittered):
    from mc_nerf_amd import ops
    dev, N = gpu_device, N_K
    d, o, g = _rays(N, 100 + Sc + G)
    z = _zgrid(Sc)
    jit = _jitter(N, Sc, g) if jittered else None
    if kind == "one":                                                   # one occupied cell: the one a sample in the middle of ray 3 sits in
        vox = _grid_of("negative", G, g)
        vox.view(-1)[V.sample_cells(o, d, z, jit, G, BMIN, BMAX)[3, Sc // 2]] = 0.5
    else:
        vox = _grid_of(kind, G, g)
    pts = V.sample_points(o, d, z, jit)
    outside = (pts.abs() > BMAX).any(-1)
    assert bool(outside.any()) and bool((~outside).any())              # the clamp runs, and so does the unclamped path
    ref_idx, ref_out = V.select(vox, 0.0, o, d, z, jit, BMIN, BMAX, SIGMA_DEFAULT)
    sentinel = torch.full((N * Sc, 2), -7, dtype=torch.int32, device=dev)
    idx, count, out_c = ops.voxel_select(_device_grid(vox, dev), 0.0, o.to(dev), d.to(dev), z.to(dev), None if jit is None else jit.to(dev),
                                         SIGMA_DEFAULT, idx=sentinel)
    k = int(count.item())
    assert k == ref_idx.shape[0]
    assert {"init": k == N * Sc, "negative": k == 0, "random": 0 < k < N * Sc, "one": 0 < k < N * Sc}[kind]
    assert torch.equal(idx[:k].cpu().long(), ref_idx)
    assert bool((idx[k:] == -7).all())                                  # nothing is written beyond the list (count 0: idx untouched)
    assert torch.equal(out_c.cpu(), ref_out)


# ---------------------------------------------------------------------------------------------------------------- 2. update
def _quantised_sigma(N, Sc, g):
    """Eight levels, so the per-cell maxima tie, with a few NaN / inf mixed in; [N,Sc,4] with sigma in channel 0."""
    sig = (torch.randint(0, 8, (N, Sc), generator=g).float() - 4.0) * 0.5
    bad = torch.randperm(N * Sc, generator=g)[:30]
    sig.view(-1)[bad[:10]] = float("nan")
    sig.view(-1)[bad[10:20]] = float("inf")
    sig.view(-1)[bad[20:]] = float("-inf")
    return torch.cat([sig.unsqueeze(-1), torch.rand(N, Sc, 3, generator=g)], -1).contiguous()


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("G", [4, 33])
def test_update_kernels_equal_the_restatement(gpu_device, G, listed):
    from mc_nerf_amd import ops
    dev, N, Sc = gpu_device, N_K, 32
    d, o, g = _rays(N, 200 + G)
    z, jit = _zgrid(Sc), _jitter(N, Sc, g)
    vox0 = _grid_of("random", G, g)
    cells = V.sample_cells(o, d, z, jit, G, BMIN, BMAX)
    if G == 4:
        assert int(torch.bincount(cells.reshape(-1), minlength=G ** 3).max()) > 200      # hundreds of collisions in a cell
    dv = lambda t: t.to(dev).contiguous()
    od, dd, zd, jd = dv(o), dv(d), dv(z), dv(jit)

    def device_update(grid, beta, sig_rgb, idx):
        if idx is None:
            ops.voxel_update(grid, beta, od, dd, zd, jd, dv(sig_rgb))
        else:                                # the list in a full-capacity buffer; the rows beyond *count hold pairs outside the grid of samples
            buf = torch.full((N * Sc, 2), 1 << 20, dtype=torch.int32, device=dev)
            buf[:idx.shape[0]] = idx.to(dev).int()
            ops.voxel_update(grid, beta, od, dd, zd, jd, dv(sig_rgb), buf, torch.tensor([idx.shape[0]], dtype=torch.int32, device=dev), N * Sc)

    steps = []
    for s_, beta in enumerate((0.1, 1.0)):                              # two updates in a row
        idx = V.select(_grid_of("random", G, g), 0.0, o, d, z, jit, BMIN, BMAX, SIGMA_DEFAULT)[0] if listed else None
        steps.append((beta, _quantised_sigma(N, Sc, g), idx))
        assert idx is None or 0 < idx.shape[0] < N * Sc
    runs = []
    for _ in range(3):
        grid, ref = _device_grid(vox0, dev), vox0
        for beta, sig_rgb, idx in steps:
            device_update(grid, beta, sig_rgb, idx)
            new = V.update(ref, beta, o, d, z, jit, sig_rgb[..., 0], BMIN, BMAX, idx)
            assert torch.equal(grid.vox.cpu(), new)
            touched = torch.zeros(G ** 3, dtype=torch.bool)
            c_, s_ = (cells.reshape(-1), sig_rgb[..., 0].reshape(-1)) if idx is None else (cells[idx[:, 0], idx[:, 1]], sig_rgb[idx[:, 0], idx[:, 1], 0])
            touched[c_[torch.isfinite(s_)]] = True
            assert bool(touched.any()) and (G == 4 or not bool(touched.all()))
            assert torch.equal(grid.vox.cpu().reshape(-1)[~touched].view(torch.int32), ref.reshape(-1)[~touched].view(torch.int32))
            assert int(grid.scratch.count_nonzero()) == 0
            ref = new
        runs.append(grid.vox.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


# ------------------------------------------------------------------------------------------------------ 3. explicit points
def test_query_sigma_and_update_sigma_equal_the_restatement(gpu_device):
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd.model import NeRF_Model
    dev, M, G = gpu_device, 1000, 33
    m = NeRF_Model(S.make_sys_param(dev, samples=32, scale=2, batch=64, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]),
                                    coarse_sampler="voxel", grid_nerf=G)).to(dev)
    g = torch.Generator().manual_seed(9)
    xyz = torch.randn(M, 3, generator=g) * 2.5                          # a part of them outside the box
    xyz[5, 1] = float("nan")
    assert bool((xyz.abs() > BMAX).any())
    vox = _grid_of("random", G, g)
    m.sigma_voxels.copy_(vox.to(dev))
    assert torch.equal(m.query_sigma(xyz.to(dev)).cpu(), V.query(vox, xyz, BMIN, BMAX))
    sig = (torch.randint(0, 8, (M,), generator=g).float() - 4.0) * 0.5
    sig[7], sig[8] = float("nan"), float("inf")
    for beta in (0.25, 1.0):
        m.update_sigma(xyz.to(dev), sig.to(dev), beta)
        vox = V.update_points(vox, xyz, sig, beta, BMIN, BMAX)
        assert torch.equal(m.sigma_voxels.cpu(), vox) and int(m.voxel_grid().scratch.count_nonzero()) == 0
        sig = sig.flip(0)
    assert torch.equal(m.query_sigma(xyz.to(dev)).cpu(), V.query(vox, xyz, BMIN, BMAX))


# ----------------------------------------------------------------------------------------------------------- models + oracle
def _voxel_model(dev, precision, batch, size="small", seed=7, **kw):
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd.model import NeRF_Model
    Sc, _, coarse, fine = SIZES[size]
    torch.manual_seed(seed)
    m = NeRF_Model(S.make_sys_param(dev, samples=Sc, scale=2, batch=batch, H=8, W=8, coarse=coarse, fine=fine, precision=precision, **kw)).to(dev)
    cfg = O.RenderCfg(near=m.near, far=m.far, samples=Sc, scale=2, coarse=O.NetCfg(coarse[0], coarse[1], tuple(coarse[2])),
                      fine=O.NetCfg(fine[0], fine[1], tuple(fine[2])), white_back=bool(m.white_back))
    pc = {k: v.detach().cpu().clone() for k, v in m.nerf_coarse.state_dict().items()}
    pf = {k: v.detach().cpu().clone() for k, v in m.nerf_fine.state_dict().items()}
    return m, cfg, pc, pf


def _list(sel):
    idx, count = sel
    return idx[:int(count.item())].cpu().long()


# ------------------------------------------------------------------------------------------------------------ 4. rebuild_voxels
def test_rebuild_voxels_is_the_coarse_net_at_the_cell_centres(gpu_device):
    """The tolerance is the fp32 one of tests/test_a_ops_gpu.py::test_mlp_fwd_dense (2e-5 on the net's outputs)."""
    dev, G = gpu_device, 8
    m, cfg, pc, _ = _voxel_model(dev, "f32", 64, coarse_sampler="voxel", grid_nerf=G)
    c = V.centres(G, BMIN, BMAX).reshape(-1, 3)
    ref = O.mlp_forward(pc, cfg.coarse, O.embed(c, 1, cfg), torch.tensor([0.0, 0.0, 1.0]).expand(c.shape[0], 3))[:, 0].reshape(G, G, G)
    got = m.rebuild_voxels(chunk=100)                                   # (6 pieces, the last one ragged)
    assert got is m.sigma_voxels and err(got, ref) < 2e-5
    assert torch.equal(m.rebuild_voxels(m.nerf_coarse), got.clone())    # one piece, the net given: the same bits


# --------------------------------------------------------------------------------------------------------------- 5. train step
def _oracle_step(pc, pf, cfg, d, o, step_r, dr, idx_c, idx_f, gt, permute):
    """The voxel-mode train render composed from the oracle: coarse inference on the coarse list, the selection weights, fine
    inference on the device's kept fine list; loss and every gradient."""
    pc = {k: v.detach().clone() for k, v in pc.items()}
    pf = {k: v.detach().clone() for k, v in pf.items()}
    undo = (lambda x: x, lambda x: x)
    if permute:
        (pc, uc), (pf, uf) = O.permute_hidden_units(pc, cfg.coarse, 1), O.permute_hidden_units(pf, cfg.fine, 2)
        undo = (uc, uf)
    for p in list(pc.values()) + list(pf.values()):
        p.requires_grad_(True)
    d_, o_ = d.clone().requires_grad_(True), o.clone().requires_grad_(True)
    N = d.shape[0]
    zc, zf = O._grids(cfg)
    z_c, z_f = zc.unsqueeze(0).expand(N, -1) + dr["jitter"], zf.unsqueeze(0).expand(N, -1) + dr["jitter"]
    rgb_c, sig_c, _, _, _ = O.inference(pc, cfg.coarse, cfg, step_r, o_, d_, z_c, dr["eps_c"], idx_render=idx_c)
    with torch.no_grad():
        w_sel = O.sigma2weights(O.deltas_of(z_c), sig_c.detach(), dr["eps_sel"])
    rgb_f, _, _, _, _ = O.inference(pf, cfg.fine, cfg, step_r, o_, d_, z_f, dr["eps_f"], idx_render=idx_f)
    loss = O.rgb_loss(rgb_c, rgb_f, gt)
    loss.backward()
    grads = {}
    for tag, p_, un in (("c", pc, undo[0]), ("f", pf, undo[1])):
        for k_, v in un({k_: p.grad for k_, p in p_.items()}).items():
            grads[f"{tag}.{k_}"] = v
    return grads, rgb_c.detach(), rgb_f.detach(), sig_c.detach(), w_sel, float(loss.detach()), d_.grad, o_.grad


@pytest.mark.parametrize("precision", MODES)
def test_voxel_train_step_matches_the_oracle_on_its_lists(gpu_device, precision):
    from mc_nerf_amd.model import MC_NeRF_Loss
    dev, N, G, beta = gpu_device, 256, 16, 0.1
    Sc = SIZES["small"][0]
    tol_rgb, tol_loss, tol_ray, tol_par, k_noise, tol_all = E2E_TOL[precision]
    m, cfg, pc, pf = _voxel_model(dev, precision, N, coarse_sampler="voxel", grid_nerf=G, voxel_warmup_epoch=0, voxel_beta=beta)
    vox0 = _ball(G)
    m.sigma_voxels.copy_(vox0.to(dev))
    d, o, g = _rays(N, 21)
    dr = dict(jitter=torch.rand(N, 1, generator=g) * (m.far - m.near) / Sc, eps_c=torch.randn(N, Sc, generator=g),
              eps_sel=torch.randn(N, Sc, generator=g), eps_f=torch.randn(N, 2 * Sc, generator=g))
    gt = torch.rand(N, 3, generator=g)
    dd, od = d.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    rgb_c, rgb_f = m.render_rays_train(dd, od, 0, 1.0, **{k: v.to(dev) for k, v in dr.items()})
    idx_c, idx_f = _list(m.last_coarse_selection), _list(m.last_selection)
    zc = O._grids(cfg)[0]
    ref_idx, _ = V.select(vox0, 0.0, o, d, zc, dr["jitter"].reshape(-1), BMIN, BMAX, SIGMA_DEFAULT)
    assert 0 < idx_c.shape[0] < N * Sc
    assert torch.equal(idx_c, ref_idx)
    ref, r_c, r_f, sig_c, _, ref_loss, ref_dd, ref_od = _oracle_step(pc, pf, cfg, d, o, 1.0, dr, idx_c, idx_f, gt, permute=False)
    assert err(rgb_c, r_c) < tol_rgb and err(rgb_f, r_f) < tol_rgb, (err(rgb_c, r_c), err(rgb_f, r_f))
    loss = MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, gt.to(dev)])
    assert abs(float(loss.detach()) - ref_loss) < tol_loss
    loss.backward()
    noise_run, _, _, _, _, _, nz_dd, nz_od = _oracle_step(pc, pf, cfg, d, o, 1.0, dr, idx_c, idx_f, gt, permute=True)
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
    # the grid afterwards: untouched cells keep their bits in every mode; f32: the restatement's update fed with the oracle's sigma
    vox1 = m.sigma_voxels.cpu()
    touched = torch.zeros(G ** 3, dtype=torch.bool)
    touched[V.sample_cells(o, d, zc, dr["jitter"].reshape(-1), G, BMIN, BMAX)[idx_c[:, 0], idx_c[:, 1]]] = True
    assert torch.equal(vox1.reshape(-1)[~touched].view(torch.int32), vox0.reshape(-1)[~touched].view(torch.int32))
    assert not torch.equal(vox1, vox0) and int(m.voxel_grid().scratch.count_nonzero()) == 0
    e_grid = None
    if precision == "f32":
        want = V.update(vox0, beta, o, d, zc, dr["jitter"].reshape(-1), sig_c, BMIN, BMAX, idx_c)
        e_grid, bound = err(vox1, want), beta * 1e-4 * float(sig_c[idx_c[:, 0], idx_c[:, 1]].abs().max())
        assert e_grid <= bound, (e_grid, bound)
    print(f"[voxel {precision}] coarse list {idx_c.shape[0]} of {N * Sc}, rgb {max(err(rgb_c, r_c), err(rgb_f, r_f)):.1e}, d_rays_d {e_d:.1e} / "
          f"d_rays_o {e_o:.1e} (oracle reorder noise {n_d:.1e} / {n_o:.1e}), worst parameter gradient {worst:.1e} of its tensor's max, "
          f"whole gradient {e_all:.1e}, grid {e_grid}")


# ----------------------------------------------------------------------------------------------- 6. warm-up and the fresh grid
def _train_run(dev, precision, N, d, o, dr, gt, cur_epoch=0, **kw):
    from mc_nerf_amd.model import MC_NeRF_Loss
    m, _, _, _ = _voxel_model(dev, precision, N, seed=4, **kw)
    rgb_c, rgb_f = m.render_rays_train(d.to(dev), o.to(dev), cur_epoch, 1.0, **{k: v.to(dev) for k, v in dr.items()})
    MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, gt.to(dev)]).backward()
    idx, count = m.last_selection
    outs = (rgb_c.detach(), rgb_f.detach(), idx[:int(count.item())].clone(), count.clone())
    return m, outs, [p.grad.detach().clone() for p in m.parameters()]


def _draws(N, Sc, seed):
    d, o, g = _rays(N, seed)
    dr = dict(jitter=torch.rand(N, 1, generator=g) * 7.0 / Sc, eps_c=torch.randn(N, Sc, generator=g),
              eps_sel=torch.randn(N, Sc, generator=g), eps_f=torch.randn(N, 2 * Sc, generator=g))
    return d, o, dr, torch.rand(N, 3, generator=g)


def test_warm_up_is_the_dense_pass_and_fills_the_grid(gpu_device):
    dev, N, precision = gpu_device, 256, "f16x3h"
    Sc = SIZES["small"][0]
    d, o, dr, gt = _draws(N, Sc, 5)
    _, a, ga = _train_run(dev, precision, N, d, o, dr, gt)
    _, _, ga2 = _train_run(dev, precision, N, d, o, dr, gt)
    _, _, ga3 = _train_run(dev, precision, N, d, o, dr, gt)
    m, b, gb = _train_run(dev, precision, N, d, o, dr, gt, coarse_sampler="voxel", grid_nerf=16, voxel_warmup_epoch=5)
    assert m.last_coarse_selection is None
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, x2, x3, y in zip(ga, ga2, ga3, gb):
        ok, info = _spread_ok(y, x, max(float((x - x2).abs().max()), float((x - x3).abs().max())))
        assert ok, info
    assert bool((m.sigma_voxels != SIGMA_INIT).any()) and int(m.voxel_grid().scratch.count_nonzero()) == 0


@pytest.mark.parametrize("precision", MODES)
def test_a_fresh_grid_lists_every_pair_and_renders_like_dense_mode(gpu_device, precision):
    dev, N = gpu_device, 256
    Sc = SIZES["small"][0]
    d, o, dr, gt = _draws(N, Sc, 6)
    _, a, _ = _train_run(dev, precision, N, d, o, dr, gt)
    m, b, _ = _train_run(dev, precision, N, d, o, dr, gt, coarse_sampler="voxel", grid_nerf=16, voxel_warmup_epoch=0)
    every = torch.stack(torch.meshgrid(torch.arange(N), torch.arange(Sc), indexing="ij"), -1).reshape(-1, 2)
    assert torch.equal(_list(m.last_coarse_selection), every)
    tol_rgb = E2E_TOL[precision][0]
    assert err(a[0], b[0]) < tol_rgb and err(a[1], b[1]) < tol_rgb, (err(a[0], b[0]), err(a[1], b[1]))


# ------------------------------------------------------------------------------------------------------- 7. default untouched
def test_dense_key_is_the_default_path_and_allocates_no_grid(gpu_device, monkeypatch):
    from mc_nerf_amd import ops
    dev, N, precision = gpu_device, 256, "f16x3h"
    Sc = SIZES["small"][0]
    d, o, dr, gt = _draws(N, Sc, 8)
    nonsense = dict(coarse_sampler="dense", voxel_beta=-7, voxel_thresh="x", voxel_warmup_epoch=None, grid_nerf=-1, boader_min=9.0, boader_max=-9.0)

    def no_grid(*a, **kw):                                              # the one place the two grids are allocated
        raise AssertionError("dense mode allocated the voxel grids")
    monkeypatch.setattr(ops, "VoxelGrid", no_grid)
    m_a, a, _ = _train_run(dev, precision, N, d, o, dr, gt)
    m_b, b, _ = _train_run(dev, precision, N, d, o, dr, gt, **nonsense)
    m_b.reserve_workspaces(N)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for m in (m_a, m_b):
        assert m.sigma_voxels is None and m._voxels is None and m.last_coarse_selection is None


# ------------------------------------------------------------------------------------------------------------------ 8. render
@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16x3h"])
def test_voxel_render_matches_the_oracle_on_its_lists(gpu_device, precision):
    dev, N, G, chunk = gpu_device, 300, 16, 128
    Sc = SIZES["small"][0]
    m, cfg, pc, pf = _voxel_model(dev, precision, chunk, coarse_sampler="voxel", grid_nerf=G, voxel_warmup_epoch=0)
    with torch.no_grad():                                               # make the density non-trivial
        m.nerf_coarse.sigma[2].bias.add_(1.5)
        m.nerf_fine.sigma[2].bias.add_(1.5)
    pc["sigma.2.bias"], pf["sigma.2.bias"] = pc["sigma.2.bias"] + 1.5, pf["sigma.2.bias"] + 1.5
    vox0 = _ball(G)
    m.sigma_voxels.copy_(vox0.to(dev))
    d, o, g = _rays(N, 33)
    zc, zf = O._grids(cfg)

    def oracle(d_, o_, e_c, e_s, e_f, idx_c, idx_f):
        with torch.no_grad():
            n = d_.shape[0]
            _, sig_c, _, _, _ = O.inference(pc, cfg.coarse, cfg, 1, o_, d_, zc.unsqueeze(0).expand(n, -1), e_c, idx_render=idx_c)
            rgb, _, depth, op, _ = O.inference(pf, cfg.fine, cfg, 1, o_, d_, zf.unsqueeze(0).expand(n, -1), e_f, idx_render=idx_f)
        return rgb, depth, op

    def check(d_, o_, e_c, e_s, e_f):
        rgb, depth, op = m.render_rays_test(d_.to(dev), o_.to(dev), m.nerf_coarse, m.nerf_fine, eps_c=e_c.to(dev), eps_sel=e_s.to(dev), eps_f=e_f.to(dev))
        idx_c, idx_f = _list(m.last_coarse_selection), _list(m.last_selection)
        assert torch.equal(idx_c, V.select(vox0, 0.0, o_, d_, zc, None, BMIN, BMAX, SIGMA_DEFAULT)[0]) and 0 < idx_c.shape[0] < d_.shape[0] * Sc
        r_rgb, r_depth, r_op = oracle(d_, o_, e_c, e_s, e_f, idx_c, idx_f)
        assert err(rgb, r_rgb) <= 1e-4 and err(depth, r_depth) <= 1e-4 and err(op, r_op) <= 1e-4, (err(rgb, r_rgb), err(depth, r_depth), err(op, r_op))
        return rgb, depth, op

    rgb, _, op = check(d, o, torch.randn(N, Sc, generator=g), torch.randn(N, Sc, generator=g), torch.randn(N, 2 * Sc, generator=g))
    assert float(op.max()) > 0.5                                        # the scene is not empty
    # render_chunked: each piece is the direct call on that piece with the same draws, bit for bit
    torch.manual_seed(99)
    rgb2, depth2, op2 = m.render_chunked(d.to(dev), o.to(dev), m.nerf_coarse, m.nerf_fine, chunk=chunk)
    torch.manual_seed(99)
    for i in range(0, N, chunk):
        n = min(chunk, N - i)
        e_c, e_s, e_f = torch.randn(n, Sc, device=dev), torch.randn(n, Sc, device=dev), torch.randn(n, 2 * Sc, device=dev)
        r, dp, op_ = check(d[i:i + n], o[i:i + n], e_c.cpu(), e_s.cpu(), e_f.cpu())
        assert torch.equal(rgb2[i:i + n], r) and torch.equal(depth2[i:i + n], dp) and torch.equal(op2[i:i + n], op_)
    assert torch.equal(m.sigma_voxels.cpu(), vox0) and int(m.voxel_grid().scratch.count_nonzero()) == 0       # rendering only queries


def test_demo_mode_builds_the_grid_from_the_loaded_coarse_net(gpu_device, tmp_path):
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd.model import NeRF_Model
    dev, G = gpu_device, 8
    trained, cfg, pc, _ = _voxel_model(dev, "f32", 64, seed=3)
    path = str(tmp_path / "ref_format.ckpt")                            # {'model_nerf': MC_Model.state_dict()}: the renderer under `nerf.`
    torch.save({"model_nerf": {f"nerf.{k}": v for k, v in trained.state_dict().items()}}, path)
    Sc, _, coarse, fine = SIZES["small"]
    torch.manual_seed(99)                                               # another init: the weights must come from the checkpoint
    demo = NeRF_Model(S.make_sys_param(dev, mode=1, demo_ckpt=path, samples=Sc, scale=2, batch=64, H=8, W=8, coarse=coarse, fine=fine,
                                       coarse_sampler="voxel", grid_nerf=G)).to(dev)
    assert demo._voxels is not None and list(demo.state_dict()) == list(trained.state_dict())
    built = demo.sigma_voxels.clone()
    assert torch.equal(built, demo.rebuild_voxels().clone())
    c = V.centres(G, BMIN, BMAX).reshape(-1, 3)
    ref = O.mlp_forward(pc, cfg.coarse, O.embed(c, 1, cfg), torch.tensor([0.0, 0.0, 1.0]).expand(c.shape[0], 3))[:, 0].reshape(G, G, G)
    assert err(built, ref) < 2e-5


# ------------------------------------------------------------------------------------------------------------- 9. convergence
# The issue's first setting, 100 warm-up steps, collapses on this scene (measured: held-out PSNR 11.05 dB against dense 22.36 dB, loss 0.3738 ->
# 0.16009, last coarse list 0.433 of N * Sc): after 100 steps the coarse net has not yet raised the raw sigma of the blobs above voxel_thresh = 0,
# their cells are emptied, and an emptied cell is never evaluated again -- a property of the update rule, not changed here.  The warm-up has to
# last until the coarse net has formed the scene: 300 of the 500 steps here.
VOXEL_WARMUP = 300


def test_voxel_sampler_converges_like_the_dense_coarse_pass(gpu_device, monkeypatch):
    """The procedural-scene loop of tests/test_y_convergence_gpu.py (500 steps, f16x3h, same seed; it passes the step index as cur_epoch),
    once dense and once with coarse_sampler = "voxel", grid_nerf = 64 and VOXEL_WARMUP dense warm-up steps followed by pruned ones: the voxel
    run's loss falls below 0.2 of its first value, its held-out PSNR is within 3 dB of the dense run's (the margin the pdf sampler's
    test gives another sampler on the same scene and seed), and the last step's coarse list is shorter than the dense grid.
    Measured (VOXEL_WARMUP = 300): dense 22.69 dB (loss 0.3738 -> mean of the last 50 steps 0.00908), voxel 22.30 dB (0.3738 -> 0.01048), the last
    step's coarse list 0.033 of N * Sc.  With 100 warm-up steps: voxel 11.05 dB (0.3738 -> 0.16009), list 0.433 (see VOXEL_WARMUP)."""
    import test_y_convergence_gpu as Y
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd.model import NeRF_Model
    steps = 500
    p_dense, f_dense, l_dense = Y._field_run(gpu_device, "f16x3h", steps)
    orig, seen = S.make_sys_param, {}
    monkeypatch.setattr(S, "make_sys_param", lambda *a, **kw: {**orig(*a, **kw), "coarse_sampler": "voxel", "grid_nerf": 64,
                                                                 "voxel_warmup_epoch": VOXEL_WARMUP})
    train = NeRF_Model.render_rays_train

    def recording(self, rays_d, *a, **kw):
        out = train(self, rays_d, *a, **kw)
        seen["last"], seen["pairs"] = self.last_coarse_selection, rays_d.shape[0] * self.samples_c
        return out
    monkeypatch.setattr(NeRF_Model, "render_rays_train", recording)
    p_vox, f_vox, l_vox = Y._field_run(gpu_device, "f16x3h", steps)
    assert seen["last"] is not None
    frac = int(seen["last"][1].item()) / seen["pairs"]
    print(f"procedural scene, {steps} steps f16x3h: held-out PSNR dense {p_dense:.2f} dB (loss {f_dense:.4f} -> {l_dense:.5f}), "
          f"voxel {p_vox:.2f} dB (loss {f_vox:.4f} -> {l_vox:.5f}); the last step's coarse list is {frac:.3f} of N * Sc")
    assert l_vox < 0.2 * f_vox
    assert abs(p_vox - p_dense) < 3.0
    assert 0.0 < frac < 1.0
