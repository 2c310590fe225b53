"""The inverse-CDF sampler kernel (mc_nerf_amd/csrc/sample_pdf.hip) beyond one 64-lane chunk and at its edges, on the case table of
tests/pdf_edge_cases.py (tests/test_pdf_edges_cpu.py shows that the table leaves the caps of `check_rows` unused):
  a. parity with the restatement (`check_rows` of tests/test_pdf_sampler_gpu.py, unchanged) into a NaN-prefilled `out` between guard rows;
  b. what the contract fixes bit for bit: draws outside [0, 1], equal draws, constant weights;
  c. the order of a row's draws does not matter;  d. rows are independent, part-filled workgroups, N = 0;
  e. the launch with more than 64 KiB of LDS;  f. NaN and inf inputs stay in their row;  g. refusals;
and one end-to-end render and train step at (Sc, I) the model accepts and no other test runs: (96, 40) and (5, 3)."""
import pytest
import torch

import pdf_edge_cases as C
from pdf_ref import sample_pdf_ref, split_rows
from test_pdf_sampler_gpu import E2E_TOL, _device_w_sel, _oracle_grads, _pdf_model, _rays, check_rows, err

pytestmark = pytest.mark.gpu
GUARD_ROWS = 3
GUARD_BITS = 0x4B1D5EED                     # (a finite float the sampler cannot produce from depths in [2, 7])
LDS_ORDER = C.BIG_LDS + [C.UNDER_BIG_LDS]   # (e): the shapes of test_large_lds_launch, in its order
OTHER_SHAPES = [s for s in C.SHAPES if s not in LDS_ORDER]


def _dev(dev, *ts):
    return [None if t is None else t.to(dev).contiguous() for t in ts]


def _guarded(dev, w, zgrid, jit, u):
    """ops.sample_pdf on device tensors into the middle rows of a larger buffer: the rows prefilled with NaN (a slot the kernel never
    wrote is seen), GUARD_ROWS rows before and behind them holding GUARD_BITS -> (the rows, the whole buffer)."""
    from mc_nerf_amd import ops
    n, T = w.shape[0], w.shape[1] + u.shape[1]
    buf = torch.empty(n + 2 * GUARD_ROWS, T, dtype=torch.float32, device=dev)
    buf.view(torch.int32).fill_(GUARD_BITS)
    rows = buf[GUARD_ROWS:GUARD_ROWS + n]
    rows.fill_(float("nan"))
    z = ops.sample_pdf(w, zgrid, jit, u, out=rows)
    assert z.data_ptr() == rows.data_ptr() and z.shape == (n, T)
    return rows, buf


def _guards_intact(buf, n):
    g = torch.cat([buf[:GUARD_ROWS], buf[GUARD_ROWS + n:]]).view(torch.int32)
    return g.numel() == 2 * GUARD_ROWS * buf.shape[1] and bool((g == GUARD_BITS).all())


def _parity(dev, Sc, I):
    """(a) and the exact expectations of (b) that sit on the table's own draws, for every case of one shape -> the share of the
    importance samples that equal the restatement's bit for bit (information, never a gate)."""
    same = total = 0
    for name, w, zgrid, jit, u in C.cases(Sc, I):
        rows, buf = _guarded(dev, *_dev(dev, w, zgrid, jit, u))
        z_all = rows.cpu()
        assert _guards_intact(buf.cpu(), C.N), f"{name}: a guard row was written"
        assert not bool(torch.isnan(z_all).any()), f"{name}: {int(torch.isnan(z_all).sum())} slots of z_all were never written"
        check_rows(z_all, w, zgrid, jit, u)
        _, zs_ref, zc = sample_pdf_ref(w, zgrid, jit, u)
        zs_dev = split_rows(z_all, zc)[0]
        same += int((zs_dev.view(torch.int32) == torch.sort(zs_ref, 1).values.view(torch.int32)).sum())
        total += zs_dev.numel()
        mid = C.edges_ref(zgrid, jit)
        if "outside" in name:
            # u = -0.5 and u = -0.0 give mid[0], u = 1.5 gives mid[Sc-2], bit for bit: ind = 0 / 1 / Sc-1, t * 0 or -0.0 * x added
            n_lo = ((u == -0.5) | ((u == 0) & torch.signbit(u))).sum(1)
            n_hi = (u == 1.5).sum(1)
            assert int(n_lo.sum()) > 0 and int(n_hi.sum()) > 0
            got_lo = (zs_dev.view(torch.int32) == mid[:, :1].contiguous().view(torch.int32)).sum(1)
            got_hi = (zs_dev.view(torch.int32) == mid[:, -1:].contiguous().view(torch.int32)).sum(1)
            assert bool((got_lo >= n_lo).all()) and bool((got_hi >= n_hi).all()), name
        if "ties" in name:
            for r in C.TIES_EQUAL_ROWS:
                assert bool((zs_dev[r].view(torch.int32) == zs_dev[r, :1].view(torch.int32)).all()), f"{name}: row {r}"
            assert C.same_bits(zs_dev[C.N - 1], mid[C.N - 1, :1].expand(I))          # (that row draws u = 0: ind = 1, t = 0)
    return same, total


# ------------------------------------------------------------------------------------------------- e. more than 64 KiB of LDS
def test_large_lds_launch(gpu_device):
    """(1021, 3) and (1023, 1) take 65600 B of LDS per workgroup: the first sampler call of this test is the launch that raises the
    kernel's dynamic-LDS limit.  (1020, 4), at 65344 B, follows.  All three through (a) and (b)."""
    for Sc, I in LDS_ORDER:
        same, total = _parity(gpu_device, Sc, I)
        print(f"[pdf edges ({Sc}, {I})] bit-equal to the restatement: {same} of {total} importance samples ({100.0 * same / total:.3f} %)")


# ------------------------------------------------------------------------------------------------------------ a, b. parity
@pytest.mark.parametrize("Sc, I", OTHER_SHAPES)
def test_kernel_matches_the_restatement_on_the_table(gpu_device, Sc, I):
    same, total = _parity(gpu_device, Sc, I)
    print(f"[pdf edges ({Sc}, {I})] bit-equal to the restatement: {same} of {total} importance samples ({100.0 * same / total:.3f} %)")


@pytest.mark.parametrize("Sc, I", C.SHAPES)
def test_constant_weights_give_the_floor(gpu_device, Sc, I):
    """Any constant weight gives the uniform pdf of all-zero weights.  c = 3 * fl(1e-5) keeps c + 1e-5 = 4 * fl(1e-5) exact (the fp32
    1e-5 ends in two zero bits), so wb, the total and the pdf scale by a power of two: bit for bit.  The pair of
    test_pdf_sampler_cpu.py::test_all_zero_weights_fall_back_to_the_floor (0 and 7.0) is bit-equal only where the restatement's is,
    and within that test's atol = 1e-6 otherwise."""
    from mc_nerf_amd import ops
    dev = gpu_device
    gen = C.gen_of(Sc, I, salt=1)
    zgrid, jit, u = C.zgrid_of(Sc), C.jitter_of(Sc, gen), torch.rand(C.N, I, generator=gen)
    c_exact = float(torch.tensor(1e-5, dtype=torch.float32) * 3)
    ws = [torch.zeros(C.N, Sc), torch.full((C.N, Sc), c_exact), torch.full((C.N, Sc), 7.0)]
    assert C.same_bits((ws[1] + 1e-5), torch.full((C.N, Sc), 1e-5) * 4)
    dz, dj, du = _dev(dev, zgrid, jit, u)
    z0, z1, z7 = [ops.sample_pdf(w.to(dev), dz, dj, du).cpu() for w in ws]
    r0, r7 = [sample_pdf_ref(w, zgrid, jit, u)[0] for w in (ws[0], ws[2])]
    check_rows(z0, ws[0], zgrid, jit, u)
    assert C.same_bits(z0, z1)
    if C.same_bits(r0, r7):
        assert C.same_bits(z0, z7)
    else:
        assert torch.allclose(r0, r7, atol=1e-6, rtol=0) and torch.allclose(z0, z7, atol=1e-6, rtol=0), (err(r0, r7), err(z0, z7))


# ------------------------------------------------------------------------------------------------------- c. order of the draws
@pytest.mark.parametrize("Sc, I", C.SHAPES)
def test_order_of_the_draws_does_not_matter(gpu_device, Sc, I):
    from mc_nerf_amd import ops
    dev = gpu_device
    gen = C.gen_of(Sc, I, salt=2)
    zgrid = C.zgrid_of(Sc)
    perm = torch.randperm(I, generator=gen)
    for wk in ("random", "peaky"):
        w, jit = C.weights_of(wk, Sc, gen), C.jitter_of(Sc, gen)
        dw, dz, dj = _dev(dev, w, zgrid, jit)
        for uk in ("random", "ties", "outside"):
            u = C.draws_of(uk, w, I, gen)
            z = ops.sample_pdf(dw, dz, dj, u.to(dev))
            for name, p in (("permuted", perm), ("reversed", torch.arange(I - 1, -1, -1))):
                z_p = ops.sample_pdf(dw, dz, dj, u[:, p].contiguous().to(dev))
                assert C.same_bits(z, z_p), f"{wk}/{uk} {name}"


# ------------------------------------------------------------------------------------------------------ d. rows, workgroups
SLICES = [(0, 1), (0, 2), (0, 3), (0, 5), (4, 257), (253, 257)]


@pytest.mark.parametrize("Sc, I", C.SHAPES)
def test_rows_are_independent_and_part_filled_workgroups_work(gpu_device, Sc, I):
    from mc_nerf_amd import ops
    dev = gpu_device
    gen = C.gen_of(Sc, I, salt=3)
    w, jit = C.weights_of("random", Sc, gen), C.jitter_of(Sc, gen)
    u = C.draws_of("ties", w, I, gen)
    dw, dz, dj, du = _dev(dev, w, C.zgrid_of(Sc), jit, u)
    full, buf = _guarded(dev, dw, dz, dj, du)
    assert _guards_intact(buf, C.N) and not bool(torch.isnan(full).any())
    assert C.same_bits(full, ops.sample_pdf(dw, dz, dj, du))               # two full calls
    for a, b in SLICES:
        for with_jitter in (True, False):
            ref = full if with_jitter else ops.sample_pdf(dw, dz, None, du)
            part, pbuf = _guarded(dev, dw[a:b].contiguous(), dz, dj[a:b].contiguous() if with_jitter else None, du[a:b].contiguous())
            assert _guards_intact(pbuf, b - a), f"rows [{a}:{b}]: a guard row was written"
            assert C.same_bits(part, ref[a:b]), f"rows [{a}:{b}], jitter {with_jitter}"
    for j in (dj[:0], None):                                               # no rays
        e = ops.sample_pdf(dw[:0].contiguous(), dz, j, du[:0].contiguous())
        assert e.shape == (0, Sc + I) and e.dtype == torch.float32 and e.device == dw.device
    keep, kbuf = _guarded(dev, dw[:0].contiguous(), dz, None, du[:0].contiguous())
    assert keep.shape == (0, Sc + I) and _guards_intact(kbuf, 0)


# --------------------------------------------------------------------------------------------- f. bad values stay in their row
@pytest.mark.parametrize("Sc, I", [(130, 33), (5, 63)])
def test_bad_values_stay_in_their_row(gpu_device, Sc, I):
    """Every store index of the kernel is < Sc + I whatever the values are: a sample goes to c + r with c = count_le(zc, Sc, z) <= Sc
    (the bisection ends after log2 steps for any comparison outcome; a NaN compares false: c = 0) and r = #{q : zs[q] < z or equal
    with q < k} <= I - 1 (q = k never counts); every sample adds 1 to one of hist[0 .. Sc], so a prefix of them is <= I and coarse
    depth j goes to j + prefix <= Sc - 1 + I.  The LDS reads take ind = count_le(cdf, Sc - 1, u) in [0, Sc - 1]: cdf[below], mid[below]
    and mid[above] at <= Sc - 2, pdf[ind - 1] only for 1 <= ind <= Sc - 2.  So a NaN or inf garbles its own row and nothing else: every
    other row and the guard rows are those of the clean call.  Nothing is claimed about rows 100 .. 103."""
    dev = gpu_device
    gen = C.gen_of(Sc, I, salt=4)
    w, jit, u = C.weights_of("random", Sc, gen), C.jitter_of(Sc, gen), torch.rand(C.N, I, generator=gen)
    zgrid = C.zgrid_of(Sc)
    clean, cbuf = _guarded(dev, *_dev(dev, w, zgrid, jit, u))
    w2, jit2, u2 = w.clone(), jit.clone(), u.clone()
    w2[100, Sc // 2] = float("nan")
    u2[101, I // 3] = float("nan")
    jit2[102] = float("nan")
    w2[103, 1] = float("inf")
    bad, bbuf = _guarded(dev, *_dev(dev, w2, zgrid, jit2, u2))
    torch.cuda.synchronize()
    assert _guards_intact(cbuf, C.N) and _guards_intact(bbuf, C.N)
    other = torch.ones(C.N, dtype=torch.bool, device=dev)
    other[100:104] = False
    assert C.same_bits(bad[other], clean[other])
    check_rows(clean, w, zgrid, jit, u)


# ------------------------------------------------------------------------------------------------------------- g. refusals
def test_refusals_leave_the_output_alone(gpu_device):
    from mc_nerf_amd import _lib, ops
    dev, N = gpu_device, 8

    def call(Sc, I, n_u=N, n_jit=N):
        out = torch.full((N, Sc + I), 3.25, device=dev)
        with pytest.raises(_lib.McnerfError):
            ops.sample_pdf(torch.rand(N, Sc, device=dev), torch.linspace(2, 6, Sc, device=dev), torch.zeros(n_jit, device=dev),
                           torch.rand(n_u, I, device=dev), out=out)
        torch.cuda.synchronize()
        assert bool((out == 3.25).all())

    call(2, 8)                      # Sc = 2: no interior bin
    call(16, 0)                     # I = 0
    call(1000, 25)                  # Sc + I = 1025
    call(16, 8, n_u=N - 1)          # u of another N
    call(16, 8, n_jit=N + 1)        # jitter of another length
    z = ops.sample_pdf(torch.rand(N, 1000, device=dev), torch.linspace(2, 6, 1000, device=dev), None, torch.rand(N, 24, device=dev))
    assert z.shape == (N, 1024) and bool((z[:, 1:] >= z[:, :-1]).all())          # ... and the bound itself is taken


# ------------------------------------------------------------------------------------- end to end at (96, 40) and (5, 3), f32
E2E_SHAPES = [(96, 40), (5, 3)]
E2E_NETS = ((4, 32, [2]), (8, 64, [4]))       # the `small` nets of test_pdf_sampler_gpu.SIZES
E2E_N = 67


@pytest.mark.parametrize("Sc, I", E2E_SHAPES)
def test_pdf_render_matches_the_oracle_at_unusual_sample_counts(gpu_device, Sc, I):
    """render_rays_test against the oracle on the device's own depth rows, the gates of
    test_pdf_sampler_gpu.py::test_pdf_render_and_render_chunked_match_the_oracle (1e-4 on rgb, depth and opacity)."""
    from oracle import mcnerf_oracle as O
    dev, N, T = gpu_device, E2E_N, Sc + I
    m, cfg, pc, pf = _pdf_model(dev, "f32", Sc, I, *E2E_NETS, N)
    d, o, g = _rays(N, 33)
    eps_c, eps_sel, eps_f = torch.randn(N, Sc, generator=g), torch.randn(N, Sc, generator=g), torch.randn(N, T, generator=g)
    u = torch.linspace(0, 1, I, device=dev).expand(N, -1).cpu()          # (the render's draws: linspace on the device)
    rgb, depth, op = m.render_rays_test(d.to(dev), o.to(dev), m.nerf_coarse, m.nerf_fine, eps_c=eps_c.to(dev), eps_sel=eps_sel.to(dev),
                                        eps_f=eps_f.to(dev))
    assert m.last_selection is None and m.last_z_all.shape == (N, T)
    z_all = m.last_z_all.cpu()
    with torch.no_grad():
        z_c = O._grids(cfg)[0].unsqueeze(0).expand(N, -1)
        _, sig_c, _, _, _ = O.inference(pc, cfg.coarse, cfg, 1, o, d, z_c, eps_c)
        w_sel = O.sigma2weights(O.deltas_of(z_c), sig_c, eps_sel)
        r_rgb, _, r_depth, r_op, _ = O.inference(pf, cfg.fine, cfg, 1, o, d, z_all, eps_f)
    w_dev = _device_w_sel(m, d, o, None, eps_c, eps_sel, 1.0)
    close = check_rows(z_all, w_dev, m.z_vals_c, None, u)
    e = (err(w_dev, w_sel), err(rgb, r_rgb), err(depth, r_depth), err(op, r_op))
    print(f"[pdf render ({Sc}, {I}) f32] w_sel {e[0]:.1e}, rgb {e[1]:.1e}, depth {e[2]:.1e}, opacity {e[3]:.1e}; samples within 2e-6: {close:.4f}")
    assert max(e) < 1e-4, e


@pytest.mark.parametrize("Sc, I", E2E_SHAPES)
def test_pdf_train_step_matches_the_oracle_at_unusual_sample_counts(gpu_device, Sc, I):
    """One render_rays_train, loss and backward against the oracle on the device's depth rows, with E2E_TOL["f32"] as
    test_pdf_sampler_gpu.py::test_pdf_train_step_matches_the_oracle_on_its_depth_rows applies it at size = "small": per tensor
    max(tol_par, 8 x the oracle's own hidden-unit reorder noise), ray gradients relative to their max, the whole gradient under
    tol_all.  Measured on MI355X (printed; errors of the worst parameter tensor relative to its max, the oracle's reorder noise of that
    tensor beside it):
      (96, 40): rgb 2.4e-7, ray gradients 3.7e-7 / 4.6e-7 (noise 1.2e-7 / 1.4e-7), worst tensor 8.5e-5 (noise 7.9e-6), whole 7.6e-7
      (5, 3):   rgb 2.4e-7, ray gradients 2.7e-7 / 3.5e-7 (noise 1.7e-7 / 2.9e-7), worst tensor 1.5e-4 (noise 3.4e-5), whole 4.1e-7
    (5, 3) is the case that moved the rgb composite backward's prefix pass to fp64 (csrc/mcnerf_composite.h): with the fp32 pass the
    fine net's sigma head missed the per-tensor gate, max(3e-4, 8 x 3.4e-5), at 4.2e-4 (sigma.2.bias) and 4.0e-4 (sigma.2.weight).  That
    gradient is the sum of dL/dsigma over the 536 fine samples, which cancels 20-fold; against the oracle run in fp64 the device was
    3.9e-4 off and the fp32 oracle 3.1e-5, and of the 3.9e-4 the forward accounts for 1.1e-4, the fp32 prefix pass for the rest, the
    weight-gradient sum for nothing.  At (32, 64), N = 256, the same tensor went from 3.0e-4 off fp64 to 5e-5."""
    from mc_nerf_amd.model import MC_NeRF_Loss
    dev, N, T = gpu_device, E2E_N, Sc + I
    tol_rgb, tol_loss, tol_ray, tol_par, k_noise, tol_all = E2E_TOL["f32"]
    m, cfg, pc, pf = _pdf_model(dev, "f32", Sc, I, *E2E_NETS, N)
    d, o, g = _rays(N, 21)
    dr = dict(jitter=torch.rand(N, 1, generator=g) * (m.far - m.near) / Sc, eps_c=torch.randn(N, Sc, generator=g),
              eps_sel=torch.randn(N, Sc, generator=g), u=torch.rand(N, I, generator=g), eps_f=torch.randn(N, T, generator=g))
    gt = torch.rand(N, 3, generator=g)
    dd, od = d.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    rgb_c, rgb_f = m.render_rays_train(dd, od, 0, 1.0, **{k: v.to(dev) for k, v in dr.items()})
    assert m.last_selection is None and m.last_z_all.shape == (N, T)
    z_all = m.last_z_all.detach().cpu()
    ref, r_c, r_f, w_sel, ref_loss, ref_dd, ref_od = _oracle_grads(pc, pf, cfg, d, o, 1.0, dr, z_all, gt, permute=False)
    w_dev = _device_w_sel(m, d, o, dr["jitter"], dr["eps_c"], dr["eps_sel"], 1.0)
    check_rows(m.last_z_all, w_dev, m.z_vals_c, dr["jitter"], dr["u"])
    loss = MC_NeRF_Loss(dict(data_img_h=8, data_img_w=8)).get_rgb_loss([rgb_c, rgb_f, gt.to(dev)])
    loss.backward()
    noise_run, _, _, _, _, nz_dd, nz_od = _oracle_grads(pc, pf, cfg, d, o, 1.0, dr, z_all, gt, permute=True)
    e_d, e_o = err(dd.grad, ref_dd) / float(ref_dd.abs().max()), err(od.grad, ref_od) / float(ref_od.abs().max())
    n_d, n_o = err(nz_dd, ref_dd) / float(ref_dd.abs().max()), err(nz_od, ref_od) / float(ref_od.abs().max())
    num = den = worst = worst_noise = 0.0
    over = []
    for tag, net in (("c", m.nerf_coarse), ("f", m.nerf_fine)):
        for k_, p in net.named_parameters():
            r_ = ref[f"{tag}.{k_}"]
            num += float(((p.grad.detach().cpu().double() - r_.double()) ** 2).sum())
            den += float((r_.double() ** 2).sum())
            scale = float(r_.abs().max())                 # relative to the tensor's own max, no floor
            e = err(p.grad, r_) / max(scale, 1e-30)
            noise = float((noise_run[f"{tag}.{k_}"] - r_).abs().max()) / max(scale, 1e-30)
            if e > worst:
                worst, worst_noise = e, noise
            if not e < max(tol_par, k_noise * noise):
                over.append((tag, k_, e, noise))
    e_all = (num / den) ** 0.5
    print(f"[pdf train ({Sc}, {I}) f32] w_sel {err(w_dev, w_sel):.1e}, rgb {max(err(rgb_c, r_c), err(rgb_f, r_f)):.1e}, loss "
          f"{abs(float(loss.detach()) - ref_loss):.1e}, d_rays_d {e_d:.1e} / d_rays_o {e_o:.1e} (oracle reorder noise {n_d:.1e} / {n_o:.1e}), "
          f"worst parameter gradient {worst:.1e} of its tensor's max (oracle reorder noise of that tensor {worst_noise:.1e}), whole gradient {e_all:.1e}")
    assert err(w_dev, w_sel) < 1e-4
    assert err(rgb_c, r_c) < tol_rgb and err(rgb_f, r_f) < tol_rgb, (err(rgb_c, r_c), err(rgb_f, r_f))
    assert abs(float(loss.detach()) - ref_loss) < tol_loss
    assert e_d < tol_ray and e_o < tol_ray, (e_d, n_d, e_o, n_o)
    assert not over, over
    assert e_all < tol_all, e_all
