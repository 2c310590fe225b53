"""The inverse-CDF fine sampler (`fine_sampler = "pdf"`) on the GPU: the sampler kernel against its torch restatement
(tests/pdf_ref.py), the per-ray depth rows of the existing kernels against their shared-grid calls, the pdf-mode render, train step
and joint camera step against the oracle run on the device's own depth rows (the oracle's general `inference()` / `composite()` take
any [N,S] z_vals), the default sampler untouched by the key, and a convergence run per sampler."""
import math

import numpy as np
import pytest
import torch

from oracle import mcnerf_oracle as O
from pdf_ref import sample_pdf_ref, split_rows

pytestmark = pytest.mark.gpu
MODES = ["f32", "f16x3", "f16x3h", "f16", "bf16"]


def err(a, b):
    return float((a.detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


def check_rows(z_all, w, zgrid, jit, u, du=1e-6):
    """z_all [N,Sc+I] of the device against the restatement: sorted, holds the coarse depths bit for bit, every importance sample
    between the restatement's samples at u - du and u + du (the inverse CDF is monotone: this absorbs the order of the CDF's sum),
    and at least 99.9 % of them within 2e-6 of the restatement's at u."""
    z_all, w, zgrid, u = z_all.cpu(), w.cpu(), zgrid.cpu(), u.cpu()
    jit = None if jit is None else jit.cpu()
    assert bool((z_all[:, 1:] >= z_all[:, :-1]).all()), "z_all is not sorted"
    _, zs_ref, zc = sample_pdf_ref(w, zgrid, jit, u)
    zs_dev, zc_found = split_rows(z_all, zc)
    assert torch.equal(zc_found, zc), "the coarse depths are not in z_all bit for bit"
    lo = torch.sort(sample_pdf_ref(w, zgrid, jit, u - du)[1], 1).values
    hi = torch.sort(sample_pdf_ref(w, zgrid, jit, u + du)[1], 1).values
    out = ~((zs_dev >= lo) & (zs_dev <= hi))
    assert not bool(out.any()), f"{int(out.sum())} importance samples outside the u +- {du} bracket"
    close = float(((zs_dev - torch.sort(zs_ref, 1).values).abs() <= 2e-6).float().mean())
    assert close >= 0.999, close
    return close


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
def _coarse_weights(dev, N, Sc, seed):
    """w_sel of a real coarse pass (random-init 4 x 128 net, jittered grid, N(0,1) selection noise)."""
    from mc_nerf_amd import ops, synthetic as S
    from mc_nerf_amd.model import NeRF_Model
    torch.manual_seed(seed)
    m = NeRF_Model(S.make_sys_param(dev, samples=Sc, scale=2, batch=N, H=8, W=8)).to(dev)
    d = torch.nn.functional.normalize(torch.randn(N, 3, device=dev), dim=-1)
    o = -4.0 * d + 0.3 * torch.randn(N, 3, device=dev)
    jit = torch.rand(N, device=dev) * (m.far - m.near) / Sc
    net, flat = m.nerf_coarse.net, m.nerf_coarse.flat_params()
    out = torch.empty(N, Sc, 4, device=dev)
    ops.mlp_fwd(net, flat, ops.pack_weights(net, flat), o, d, m.z_vals_c, jit, m.emmbedding_xyz.barf_weights_on(1, dev, pad=10), out)
    w_sel = ops.composite_fwd(out, d, m.z_vals_c, jit, torch.randn(N, Sc, device=dev), torch.randn(N, Sc, device=dev))[3]
    return w_sel, m.z_vals_c, jit


@pytest.mark.parametrize("wkind", ["random", "zero", "onehot", "coarse"])
@pytest.mark.parametrize("I", [64, 128, 192])
@pytest.mark.parametrize("Sc", [32, 64])
def test_sampler_kernel_matches_the_restatement(gpu_device, Sc, I, wkind):
    from mc_nerf_amd import ops
    dev, N = gpu_device, 4096
    g = torch.Generator(device=dev).manual_seed(Sc * 1000 + I)
    zgrid = torch.linspace(2.0, 6.0, Sc, device=dev)
    jit = torch.rand(N, device=dev, generator=g) * 4.0 / Sc
    if wkind == "random":
        w = torch.rand(N, Sc, device=dev, generator=g)
    elif wkind == "zero":
        w = torch.zeros(N, Sc, device=dev)
    elif wkind == "onehot":
        w = torch.nn.functional.one_hot(torch.randint(0, Sc, (N,), device=dev, generator=g), Sc).float()
    else:
        w, zgrid, jit = _coarse_weights(dev, N, Sc, seed=I)
    for ukind in ("random", "linspace"):
        u = torch.rand(N, I, device=dev, generator=g) if ukind == "random" else torch.linspace(0, 1, I, device=dev).expand(N, -1).contiguous()
        z_all = ops.sample_pdf(w.contiguous(), zgrid, jit, u)
        assert z_all.shape == (N, Sc + I)
        check_rows(z_all, w, zgrid, jit, u)
    z0 = ops.sample_pdf(w.contiguous(), zgrid, None, u)                    # no jitter: the bare grid
    check_rows(z0, w, zgrid, None, u)


# ------------------------------------------------------------------------------- 2. depth rows against the shared-grid call
def _spread_ok(a, b, spread):
    """a against b within twice the run-to-run spread of b's own computation, or within 1e-6 of b's max (float-atomic sums: the
    grid call's own runs differ by up to ~0.8e-6 of the max in the ray gradients, so 1e-6 alone cannot be a cap)."""
    scale = float(b.abs().max())
    e = float((a - b).abs().max())
    return e <= max(2.0 * spread, 1e-6 * scale), (e, spread, scale)


@pytest.mark.parametrize("precision", MODES)
def test_depth_rows_equal_the_grid_call(gpu_device, precision):
    """z_all := zgrid + jitter fed as rows (jitter None) reproduces the grid call: the forward, both composites, the saved operands
    and the dX chain's workspaces bit for bit; the ray gradients and the weight gradients (float atomics, an order that changes
    from run to run) as closely as two runs of the grid call agree, and never worse than 1e-6 of each tensor's max."""
    from mc_nerf_amd import ops, synthetic as S
    from mc_nerf_amd.model import NeRF_Model
    dev, N = gpu_device, 512
    torch.manual_seed(5)
    m = NeRF_Model(S.make_sys_param(dev, samples=64, scale=2, batch=N, H=8, W=8, precision=precision)).to(dev)
    net, flat = m.nerf_fine.net, m.nerf_fine.flat_params()
    packed = ops.pack_weights(net, flat, precision=precision)
    zgrid = m.z_vals_f
    S_ = zgrid.numel()
    d = torch.nn.functional.normalize(torch.randn(N, 3, device=dev), dim=-1)
    o = -4.0 * d + 0.3 * torch.randn(N, 3, device=dev)
    jit = torch.rand(N, device=dev) * 7.0 / 64
    rows = (zgrid.unsqueeze(0) + jit.unsqueeze(1)).contiguous()
    barf_w = m.emmbedding_xyz.barf_weights_on(1, dev, pad=10)
    eps, eps_sel = torch.randn(N, S_, device=dev), torch.randn(N, S_, device=dev)
    d_rgb = torch.randn(N, 3, device=dev) * 1e-2

    def run(use_rows):
        zg, jt, kw = (None, None, dict(z_rows=rows)) if use_rows else (zgrid, jit, {})
        save = ops.alloc_save(net, N * S_, dev, precision)
        for t in (save.act, save.enc, save.sh, save.mask):
            t.zero_()
        out = torch.empty(N, S_, 4, device=dev)
        ops.mlp_fwd(net, flat, packed, o, d, zg, jt, barf_w, out, save=save, precision=precision, **kw)
        comp = ops.composite_fwd(out, d, zg, jt, eps, eps_sel, True, want_depth=True, **kw)
        d_out, gmax = ops.composite_bwd(out, zg, jt, eps, d_rgb, True, want_gmax=True, **kw)
        dy, dsh = ops.alloc_grad_ws(net, save, precision)
        dy.zero_(), dsh.zero_()
        d_o, d_d = torch.zeros(N, 3, device=dev), torch.zeros(N, 3, device=dev)
        ops.mlp_bwd(net, flat, packed, o, d, zg, jt, barf_w, out, d_out, save, dy, dsh, d_o, d_d, precision=precision, gmax=gmax, **kw)
        grads = torch.zeros_like(flat)
        ops.mlp_dw(net, save, dy, dsh, grads, N * S_, precision=precision, gmax=gmax)
        torch.cuda.synchronize()
        exact = [out, *comp, d_out, gmax, save.act, save.enc, save.sh, save.mask, dy, dsh]
        return exact, (d_o, d_d, grads)

    e1, a1 = run(False)
    _, a2 = run(False)
    _, a4 = run(False)
    e3, a3 = run(True)
    for i, (x, y) in enumerate(zip(e1, e3)):
        assert torch.equal(x, y), f"tensor {i} differs between the grid call and the depth rows"
    for x1, x2, x4, x3 in zip(a1, a2, a4, a3):
        spread = max(float((x1 - x2).abs().max()), float((x1 - x4).abs().max()))
        ok, info = _spread_ok(x3, x1, spread)
        assert ok, info


# --------------------------------------------------------------------------------------------- oracle on the device's z_all
def _pdf_oracle(pc, pf, cfg, d, o, step_r, jit, eps_c, eps_sel, eps_f, z_all):
    """The pdf-mode train render composed from the oracle: coarse inference on grid + jitter, the selection weights, the fine
    inference on the given depth rows (a constant: no gradient through the sampler)."""
    N = d.shape[0]
    zc = O._grids(cfg)[0]
    z_c = zc.unsqueeze(0).expand(N, -1) + jit.reshape(N, 1)
    rgb_c, sig_c, _, _, _ = O.inference(pc, cfg.coarse, cfg, step_r, o, d, z_c, eps_c)
    with torch.no_grad():
        w_sel = O.sigma2weights(O.deltas_of(z_c), sig_c.detach(), eps_sel)
    rgb_f, _, depth_f, op_f, _ = O.inference(pf, cfg.fine, cfg, step_r, o, d, z_all, eps_f)
    return rgb_c, rgb_f, w_sel, depth_f, op_f


def _oracle_grads(pc, pf, cfg, d, o, step_r, dr, z_all, gt, permute):
    pc = {k: v.detach().clone() for k, v in pc.items()}
    pf = {k: v.detach().clone() for k, v in pf.items()}
    undo = (lambda x: x, lambda x: x)
    if permute:
        (pc, uc), (pf, uf) = O.permute_hidden_units(pc, cfg.coarse, 1), O.permute_hidden_units(pf, cfg.fine, 2)
        undo = (uc, uf)
    for p in list(pc.values()) + list(pf.values()):
        p.requires_grad_(True)
    d_ = d.clone().requires_grad_(True)
    o_ = o.clone().requires_grad_(True)
    rgb_c, rgb_f, w_sel, _, _ = _pdf_oracle(pc, pf, cfg, d_, o_, step_r, dr["jitter"], dr["eps_c"], dr["eps_sel"], dr["eps_f"], z_all)
    loss = O.rgb_loss(rgb_c, rgb_f, gt)
    loss.backward()
    out = {}
    for tag, p_, un in (("c", pc, undo[0]), ("f", pf, undo[1])):
        for k_, v in un({k_: p.grad for k_, p in p_.items()}).items():
            out[f"{tag}.{k_}"] = v
    return out, rgb_c.detach(), rgb_f.detach(), w_sel, float(loss.detach()), d_.grad, o_.grad


# per mode: (rgb, loss, ray gradients / max, per-tensor floor, multiple of the oracle's reorder noise, whole gradient) -- the gates of
# test_model_gpu.py::test_sh_degree_topology_matches_reference; the single-pass 16-bit modes are held to the whole-gradient gate
E2E_TOL = {"f32": (1e-4, 1e-5, 1e-4, 3e-4, 8.0, 1e-5), "f16x3": (1e-4, 1e-5, 1e-4, 1.5e-2, 8.0, 1e-5),
           "f16x3h": (1e-4, 1e-5, 1e-4, 1.5e-2, 8.0, 2e-4), "f16": (1e-4, 1e-3, 1e-1, None, None, 1e-2), "bf16": (6e-4, 1e-3, 3e-1, None, None, 6e-2)}
SIZES = {"small": (32, 64, (4, 32, [2]), (8, 64, [4])), "default": (64, 128, (4, 128, [2]), (8, 256, [4]))}


def _pdf_model(dev, precision, Sc, I, coarse, fine, batch, seed=7, **kw):
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd.model import NeRF_Model
    torch.manual_seed(seed)
    sp = S.make_sys_param(dev, samples=Sc, scale=2, batch=batch, H=8, W=8, coarse=coarse, fine=fine, precision=precision,
                          fine_sampler="pdf", n_importance=I, **kw)
    m = NeRF_Model(sp).to(dev)
    cfg = O.RenderCfg(near=m.near, far=m.far, samples=Sc, scale=2, coarse=O.NetCfg(coarse[0], coarse[1], tuple(coarse[2])),
                      fine=O.NetCfg(fine[0], fine[1], tuple(fine[2])), white_back=bool(m.white_back))
    pc = {k: v.detach().cpu().clone() for k, v in m.nerf_coarse.state_dict().items()}
    pf = {k: v.detach().cpu().clone() for k, v in m.nerf_fine.state_dict().items()}
    return m, cfg, pc, pf


def _rays(N, seed, near_far=(2.0, 6.0)):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    o = -4.0 * d + 0.3 * torch.randn(N, 3, generator=g)
    return d, o, g


def _device_w_sel(m, d, o, jit, eps_c, eps_sel, step_r):
    """The selection weights the model's coarse pass fed to its sampler, recomputed with the same kernels and inputs (the coarse
    forward and the composite are deterministic): the input of the sampler check (1) on the device's own rows."""
    from mc_nerf_amd import ops
    dev, prec = m.z_vals_c.device, m.settings.precision
    net, flat = m.nerf_coarse.net, m.nerf_coarse.flat_params()
    N = d.shape[0]
    jit = None if jit is None else jit.reshape(-1).to(dev).contiguous()
    out = torch.empty(N, m.samples_c, 4, device=dev)
    d, o = d.to(dev).contiguous(), o.to(dev).contiguous()
    ops.mlp_fwd(net, flat, ops.pack_weights(net, flat, precision=prec), o, d, m.z_vals_c, jit,
                m.emmbedding_xyz.barf_weights_on(step_r, dev, pad=10), out, precision=prec)
    return ops.composite_fwd(out, d, m.z_vals_c, jit, eps_c.to(dev).contiguous(), eps_sel.to(dev).contiguous(), m.white_back)[3]


# ----------------------------------------------------------------------------------------------------- 3. end to end, train
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("size", ["small", "default"])
def test_pdf_train_step_matches_the_oracle_on_its_depth_rows(gpu_device, size, precision):
    from mc_nerf_amd.model import MC_NeRF_Loss
    dev, N = gpu_device, 256
    Sc, I, coarse, fine = SIZES[size]
    tol_rgb, tol_loss, tol_ray, tol_par, k_noise, tol_all = E2E_TOL[precision]
    m, cfg, pc, pf = _pdf_model(dev, precision, Sc, I, coarse, fine, N)
    d, o, g = _rays(N, 21)
    T = Sc + I
    dr = dict(jitter=torch.rand(N, 1, generator=g) * (m.far - m.near) / Sc, eps_c=torch.randn(N, Sc, generator=g),
              eps_sel=torch.randn(N, Sc, generator=g), u=torch.rand(N, I, generator=g), eps_f=torch.randn(N, T, generator=g))
    gt = torch.rand(N, 3, generator=g)
    dd, od = d.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    rgb_c, rgb_f = m.render_rays_train(dd, od, 0, 1.0, **{k: v.to(dev) for k, v in dr.items()})
    assert m.last_selection is None and m.last_z_all.shape == (N, T)
    z_all = m.last_z_all.detach().cpu()
    ref, r_c, r_f, w_sel, ref_loss, ref_dd, ref_od = _oracle_grads(pc, pf, cfg, d, o, 1.0, dr, z_all, gt, permute=False)
    # the device's rows: the sampler check (1) on the selection weights of the device's coarse pass
    w_dev = _device_w_sel(m, d, o, dr["jitter"], dr["eps_c"], dr["eps_sel"], 1.0)
    check_rows(m.last_z_all, w_dev, m.z_vals_c, dr["jitter"], dr["u"])
    if precision in ("f32", "f16x3", "f16x3h"):
        assert err(w_dev, w_sel) < 1e-4
    assert err(rgb_c, r_c) < tol_rgb and err(rgb_f, r_f) < tol_rgb, (err(rgb_c, r_c), err(rgb_f, r_f))
    loss = MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, gt.to(dev)])
    assert abs(float(loss.detach()) - ref_loss) < tol_loss
    loss.backward()
    # ray gradients relative to their max (no floor): 1e-4 at the small nets; the full-size nets (sums over 192 samples through the
    # 8 x 256 chain and the 2^9-frequency encoding) are measured at 1.1e-4 (f32) and 2.8e-4 (f16x3 / f16x3h) of the max and gated at
    # 5e-4 -- the oracle's own hidden-unit reorder noise there (printed) is 1e-5: it does not perturb the sample positions
    noise_run, _, _, _, _, nz_dd, nz_od = _oracle_grads(pc, pf, cfg, d, o, 1.0, dr, z_all, gt, permute=True)
    e_d, e_o = err(dd.grad, ref_dd) / float(ref_dd.abs().max()), err(od.grad, ref_od) / float(ref_od.abs().max())
    n_d, n_o = err(nz_dd, ref_dd) / float(ref_dd.abs().max()), err(nz_od, ref_od) / float(ref_od.abs().max())
    tr = max(tol_ray, 5e-4) if size == "default" else tol_ray
    if size == "default" and precision == "f32":
        tol_par = 1e-3          # (measured 4.9e-4 of the tensor's max: the coarse net's layer 2, the same coarse pass as the threshold path's)
    assert e_d < tr and e_o < tr, (e_d, n_d, e_o, n_o)
    num = den = worst = 0.0
    for tag, net in (("c", m.nerf_coarse), ("f", m.nerf_fine)):
        for k_, p in net.named_parameters():
            r_ = ref[f"{tag}.{k_}"]
            num += float(((p.grad.detach().cpu().double() - r_.double()) ** 2).sum())
            den += float((r_.double() ** 2).sum())
            scale = float(r_.abs().max())                 # relative to the tensor's own max, no floor
            e = err(p.grad, r_) / max(scale, 1e-30)
            noise = float((noise_run[f"{tag}.{k_}"] - r_).abs().max()) / max(scale, 1e-30)
            worst = max(worst, e)
            if tol_par is not None:
                assert e < max(tol_par, k_noise * noise), (tag, k_, e, noise)
    e_all = (num / den) ** 0.5
    assert e_all < tol_all, e_all
    print(f"[pdf {size} {precision}] rgb {max(err(rgb_c, r_c), err(rgb_f, r_f)):.1e}, d_rays_d {e_d:.1e} / d_rays_o {e_o:.1e} (oracle reorder "
          f"noise {n_d:.1e} / {n_o:.1e}), worst parameter gradient "
          f"{worst:.1e} of its tensor's max, whole gradient {e_all:.1e}")


# ---------------------------------------------------------------------------------------------------- 4. end to end, render
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_pdf_render_and_render_chunked_match_the_oracle(gpu_device, precision):
    dev, N = gpu_device, 300
    Sc, I, coarse, fine = SIZES["default"]
    m, cfg, pc, pf = _pdf_model(dev, precision, Sc, I, coarse, fine, 128)
    d, o, g = _rays(N, 33)
    T = Sc + I
    eps_c, eps_sel, eps_f = torch.randn(N, Sc, generator=g), torch.randn(N, Sc, generator=g), torch.randn(N, T, generator=g)
    u = torch.linspace(0, 1, I, device=dev).expand(N, -1).cpu()          # (the render's draws: linspace on the device)

    def oracle(d_, o_, e_c, e_s, e_f, z_all):
        with torch.no_grad():
            n = d_.shape[0]
            z_c = O._grids(cfg)[0].unsqueeze(0).expand(n, -1)
            _, sig_c, _, _, _ = O.inference(pc, cfg.coarse, cfg, 1, o_, d_, z_c, e_c)
            w_sel = O.sigma2weights(O.deltas_of(z_c), sig_c, e_s)
            rgb, _, depth, op, _ = O.inference(pf, cfg.fine, cfg, 1, o_, d_, z_all, e_f)
        return rgb, depth, op, w_sel

    rgb, depth, op = m.render_rays_test(d.to(dev), o.to(dev), m.nerf_coarse, m.nerf_fine, eps_c=eps_c.to(dev), eps_sel=eps_sel.to(dev),
                                        eps_f=eps_f.to(dev))
    assert m.last_selection is None
    z_all = m.last_z_all.cpu()
    r_rgb, r_depth, r_op, w_sel = oracle(d, o, eps_c, eps_sel, eps_f, z_all)
    w_dev = _device_w_sel(m, d, o, None, eps_c, eps_sel, 1.0)
    check_rows(z_all, w_dev, m.z_vals_c, None, u)
    assert err(w_dev, w_sel) < 1e-4
    assert err(rgb, r_rgb) < 1e-4 and err(depth, r_depth) < 1e-4 and err(op, r_op) < 1e-4, (err(rgb, r_rgb), err(depth, r_depth), err(op, r_op))
    # render_chunked: the draws of each chunk come from the device generator in render_rays_test's order; replay them
    chunk = 128
    torch.manual_seed(99)
    rgb2, depth2, op2 = m.render_chunked(d.to(dev), o.to(dev), m.nerf_coarse, m.nerf_fine, chunk=chunk)
    torch.manual_seed(99)
    for i in range(0, N, chunk):
        n = min(chunk, N - i)
        e_c, e_s, e_f = (torch.randn(n, Sc, device=dev), torch.randn(n, Sc, device=dev), torch.randn(n, T, device=dev))
        with torch.no_grad():
            m.render_rays_test(d[i:i + n].to(dev), o[i:i + n].to(dev), m.nerf_coarse, m.nerf_fine, eps_c=e_c, eps_sel=e_s, eps_f=e_f)
        r_rgb, r_depth, r_op, _ = oracle(d[i:i + n], o[i:i + n], e_c.cpu(), e_s.cpu(), e_f.cpu(), m.last_z_all.cpu())
        assert err(rgb2[i:i + n], r_rgb) < 1e-4 and err(depth2[i:i + n], r_depth) < 1e-4 and err(op2[i:i + n], r_op) < 1e-4


# ------------------------------------------------------------------------------------------------------------ 5. joint stage
def test_pdf_mc_model_joint_step_pose_gradient_matches_the_oracle(gpu_device):
    """One GLOBAL_OPTIM step of MC_Model in pdf mode (f16x3h): the `weights_pose` gradient of the drawn camera against the same step
    composed from the oracle on the device's depth rows (as tests/test_model_gpu.py::test_mc_model_joint_optimisation_step_matches_oracle)."""
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss
    dev = gpu_device
    H, W, B, cam, Sc, I = 24, 32, 96, 7, 32, 64
    sp = S.make_sys_param(dev, samples=Sc, scale=2, batch=B, H=H, W=W, coarse=(4, 32, [2]), fine=(8, 64, [4]),
                          barf_start=0.2, barf_end=0.9, precision="f16x3h", fine_sampler="pdf", n_importance=I)
    torch.manual_seed(3)
    model = MC_Model(sp).to(dev)
    S.init_cameras_near_gt(model, noise=0.02, seed=1)
    g = torch.Generator().manual_seed(11)
    idx = torch.randperm(H * W, generator=g)[:B]
    draws = dict(jitter=torch.rand(B, 1, generator=g) * 7.0 / Sc, eps_c=torch.randn(B, Sc, generator=g),
                 eps_sel=torch.randn(B, Sc, generator=g), u=torch.rand(B, I, generator=g), eps_f=torch.randn(B, Sc + I, generator=g))
    model.sample_pixels = lambda npix: idx.to(dev)
    orig = model.nerf.render_rays_train
    model.nerf.render_rays_train = lambda d, o, e, r, only_coarse=False: orig(
        d, o, e, r, only_coarse, **{k: v.to(dev) for k, v in draws.items()})
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0], seed=2)
    gt_img = torch.rand(1, H * W, 3, generator=g)
    data = (gt_img, torch.tensor([cam]), wpts, pts, wpts, pts)
    cur_ratio = 0.6
    loss_dict, _, _, _ = model(data, 20, "GLOBAL_OPTIM_EPOCH", cur_ratio)
    loss = MC_NeRF_Loss(sp)(loss_dict, "GLOBAL_OPTIM_EPOCH")
    loss.backward()
    z_all = model.nerf.last_z_all.detach().cpu()
    assert model.nerf.last_selection is None and z_all.shape == (B, Sc + I)

    cfg = O.RenderCfg(samples=Sc, scale=2, coarse=O.NetCfg(4, 32, (2,)), fine=O.NetCfg(8, 64, (4,)), barf_mode=True,
                      barf_start=0.2, barf_end=0.9)
    cp = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in model.named_parameters()}
    pc = {k[len("nerf.nerf_coarse."):]: v for k, v in cp.items() if k.startswith("nerf.nerf_coarse.")}
    pf = {k[len("nerf.nerf_fine."):]: v for k, v in cp.items() if k.startswith("nerf.nerf_fine.")}
    K = O.intrinsics_from_weights(H, W, cp["weights_fx"], cp["weights_fy"], cp["weights_ux"], cp["weights_uy"])
    pose = O.se3_to_SE3(cp["weights_pose"])
    calib = O.se3_to_SE3(cp["weights_pose_intr"])
    camp = torch.cat([wpts, torch.ones_like(wpts[..., :1])], -1) @ calib.unsqueeze(0).transpose(-2, -1)
    pix = camp @ K.unsqueeze(0).transpose(-2, -1)
    rep = pix[..., :2] / pix[..., 2:]
    l_intr = ((rep[..., 0] - pts[..., 0]) / W).pow(2).mean() + ((rep[..., 1] - pts[..., 1]) / H).pow(2).mean()
    d, o = O.get_rays_at(pose[cam], torch.linalg.inv(K[cam]), idx, W)
    rgb_c, rgb_f, _, _, _ = _pdf_oracle(pc, pf, cfg, d, o, cur_ratio, draws["jitter"], draws["eps_c"], draws["eps_sel"], draws["eps_f"], z_all)
    ref_loss = l_intr / (l_intr.detach() + 1e-8) + O.rgb_loss(rgb_c, rgb_f, gt_img.reshape(-1, 3)[idx])
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < 2e-5
    gp, rp = model.weights_pose.grad[cam].cpu(), cp["weights_pose"].grad[cam]
    assert float(rp.abs().max()) > 0
    assert err(gp, rp) < 1e-3 * float(rp.abs().max()), (err(gp, rp), float(rp.abs().max()))


# ---------------------------------------------------------------------------------------------------------- 6. default untouched
def test_threshold_key_is_the_default_path(gpu_device):
    """The same model and draws with the key absent and with fine_sampler = "threshold": outputs and selection bit for bit, gradients
    as close as two runs of the key-less model (weight-gradient atomics)."""
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd.model import MC_NeRF_Loss, NeRF_Model
    dev, N = gpu_device, 1024
    d, o, g = _rays(N, 5)
    dr = dict(jitter=torch.rand(N, 1, generator=g) * 7.0 / 64, eps_c=torch.randn(N, 64, generator=g),
              eps_sel=torch.randn(N, 64, generator=g), eps_f=torch.randn(N, 128, generator=g))
    gt = torch.rand(N, 3, generator=g).to(dev)

    def run(**kw):
        torch.manual_seed(4)
        m = NeRF_Model(S.make_sys_param(dev, samples=64, scale=2, batch=N, H=8, W=8, precision="f16x3h", **kw)).to(dev)
        rgb_c, rgb_f = m.render_rays_train(d.to(dev), o.to(dev), 0, 1.0, **{k: v.to(dev) for k, v in dr.items()})
        MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, gt]).backward()
        idx, count = m.last_selection
        k = int(count.item())
        grads = [p.grad.detach().clone() for p in m.parameters()]
        return (rgb_c.detach(), rgb_f.detach(), idx[:k].clone(), count.clone()), grads

    a, ga = run()
    a2, ga2 = run()
    a3, ga3 = run()
    b, gb = run(fine_sampler="threshold", n_importance=17)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, x2, x3, y in zip(ga, ga2, ga3, gb):
        ok, info = _spread_ok(y, x, max(float((x - x2).abs().max()), float((x - x3).abs().max())))
        assert ok, info


# ------------------------------------------------------------------------------------------------------------- 7. convergence
PDF_PSNR_FLOOR_DB = 20.0      # ~2 dB under the measured pdf run (22.0 dB; printed by the test)


def test_pdf_sampler_converges_like_the_threshold_sampler(gpu_device, monkeypatch):
    """The procedural-scene loop of tests/test_y_convergence_gpu.py (500 steps, f16x3h, same seed), once per sampler: the pdf run's
    held-out PSNR is above its floor and within 3 dB of the threshold run's.  Measured: threshold 22.47 dB (loss 0.3738 -> mean of the
    last 50 steps 0.00830), pdf 22.03 dB (0.3739 -> 0.00965)."""
    import test_y_convergence_gpu as Y
    from mc_nerf_amd import synthetic as S
    steps = 500
    p_thr, f_thr, l_thr = Y._field_run(gpu_device, "f16x3h", steps)
    orig = S.make_sys_param
    monkeypatch.setattr(S, "make_sys_param", lambda *a, **kw: {**orig(*a, **kw), "fine_sampler": "pdf", "n_importance": 128})
    p_pdf, f_pdf, l_pdf = Y._field_run(gpu_device, "f16x3h", steps)
    print(f"procedural scene, {steps} steps f16x3h: held-out PSNR threshold {p_thr:.2f} dB (loss {f_thr:.4f} -> {l_thr:.5f}), "
          f"pdf {p_pdf:.2f} dB (loss {f_pdf:.4f} -> {l_pdf:.5f})")
    assert l_pdf < 0.2 * f_pdf
    assert p_pdf > PDF_PSNR_FLOOR_DB
    assert abs(p_pdf - p_thr) < 3.0
