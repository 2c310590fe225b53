"""The bounds library's entry points (include/mcnerf_box.h; csrc/ray_bounds.hip) on the GPU.

  0. the listed pass on rows   mlp_fwd / mlp_bwd / mlp_dw with `idx` + `z_rows` against `idx` + `zgrid` + `jitter` (existing kernels,
                               the combination the threshold fine pass of "aabb" mode runs and no other test does), all five modes;
  1. ray_depths                z_c, z_f and span against the torch-CPU fp32 restatement (tests/ray_bounds_ref.py), bit for bit, on the
                               hand-made rays; against fp64 within the bound derived from the roundings;
  2. sample_pdf on rows        the grid entry point's bits on rows fl(zgrid + jitter); the sampler's restatement on clipped rows;
  3. voxel select / update     the grid entry points' results on rows fl(zgrid + jitter); the restatement on clipped rows.
"""
import pytest
import torch

import ray_bounds_ref as B
import voxel_ref as V
from pdf_ref import split_rows
from test_mlpx3h_gpu import alloc_ff, indexed_case
from test_pdf_sampler_gpu import MODES, _spread_ok

pytestmark = pytest.mark.gpu
BMIN, BMAX, SIGMA_INIT, SIGMA_DEFAULT = -3.5, 3.5, 30.0, -20.0


def _ops():
    from mc_nerf_amd import ops
    return ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# -------------------------------------------------------------------------------------------------- 0. the listed pass on rows
COUNTS = (1, 127, 128, 129, 255, 256, 257)      # the pass edges of every family: 128 rows (f16x3 from width 128, f32 tiles), 256 (the 16-bit chains, f16x3 below)
CAP = 320


def _run_listed(dev, c, precision, count, d_out, gmax, rows):
    """tests/test_mlpx3h_gpu.py::run_chain with the depths as `rows` [N,S] (zgrid and jitter None) when given."""
    ops = _ops()
    net = c.net
    packed = ops.pack_weights(net, c.flat, precision=precision)
    idx_d = torch.zeros(CAP, 2, dtype=torch.int32, device=dev)
    idx_d[:] = c.idx[:CAP].to(torch.int32).to(dev)
    cnt = torch.tensor([count], dtype=torch.int32, device=dev)
    od, dd, zd, jd = c.dev_in
    zg, jt, kw = (zd, jd, {}) if rows is None else (None, None, dict(z_rows=rows))
    out = torch.full((c.N, c.S, 4), 7.0, device=dev)
    grads, d_o, d_d = torch.zeros_like(c.flat), torch.zeros(c.N, 3, device=dev), torch.zeros(c.N, 3, device=dev)
    save, dy, dsh = alloc_ff(ops, net, CAP, dev, precision)
    ops.mlp_fwd(net, c.flat, packed, od, dd, zg, jt, c.bw, out, idx=idx_d, count=cnt, max_rows=CAP, save=save, precision=precision, **kw)
    ops.mlp_bwd(net, c.flat, packed, od, dd, zg, jt, c.bw, out, d_out, save, dy, dsh, d_o, d_d, idx=idx_d, count=cnt, max_rows=CAP,
                precision=precision, gmax=gmax, **kw)
    ops.mlp_dw(net, save, dy, dsh, grads, CAP, count=cnt, precision=precision, gmax=gmax)
    torch.cuda.synchronize()
    return [out, save.act, save.enc, save.sh, save.mask, dy, dsh], [d_o, d_d, grads]


@pytest.mark.parametrize("precision", MODES)
def test_listed_pass_on_rows_equals_the_listed_pass_on_the_grid(gpu_device, precision):
    """The smallest net of the existing op tests (tests/test_mlpx3h_gpu.py: NETS[32], 4 x 32 with a skip layer, BARF on), a list of 60 %
    of a 29 x 40 grid, counts at the pass edges.  The output and every workspace (0xFF-filled before the launch) bit for bit; the ray
    and weight gradients, which every family accumulates with float atomics in an order that changes from run to run, by the gate of
    tests/test_pdf_sampler_gpu.py::test_depth_rows_equal_the_grid_call (`_spread_ok`: twice the spread of the grid call's own runs, or
    1e-6 of the tensor's max)."""
    dev = gpu_device
    c = indexed_case(dev, 32, N=29, S=40)
    assert c.K >= CAP
    rows = (c.zg.unsqueeze(0) + c.jitter).contiguous()                  # fl(zgrid[j] + jitter[n]) on the CPU
    d_out = torch.zeros(c.N, c.S, 4, device=dev)
    d_out[c.idx[:, 0].to(dev), c.idx[:, 1].to(dev)] = (torch.randn(c.K, 4, generator=c.gen) * 1e-4).to(dev)
    gmax = d_out.abs().max().reshape(1).view(torch.int32)
    rows_d = rows.to(dev)
    assert same_bits(rows_d, c.dev_in[2].unsqueeze(0) + c.dev_in[3].unsqueeze(1))      # ... is the device's own sum
    worst = 0.0
    for count in COUNTS:
        e1, a1 = _run_listed(dev, c, precision, count, d_out, gmax, None)
        _, a2 = _run_listed(dev, c, precision, count, d_out, gmax, None)
        _, a4 = _run_listed(dev, c, precision, count, d_out, gmax, None)
        e3, a3 = _run_listed(dev, c, precision, count, d_out, gmax, rows_d)
        for i, (x, y) in enumerate(zip(e1, e3)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{precision} count {count}: tensor {i} differs between the grid call and the rows"
        assert float(a1[2].abs().max()) > 0 and float(a1[0].abs().max()) > 0
        for x1, x2, x4, x3 in zip(a1, a2, a4, a3):
            spread = max(float((x1 - x2).abs().max()), float((x1 - x4).abs().max()))
            ok, info = _spread_ok(x3, x1, spread)
            assert ok, (precision, count, info)
            worst = max(worst, info[0] / info[2])
    print(f"[listed pass on rows {precision}] {len(COUNTS)} counts: workspaces bit-equal; gradients within {worst:.1e} of their tensor's max of the grid call's")


# ------------------------------------------------------------------------------------------------------------- 1. ray_depths
def _depths_case(N, Sc, Sf, jittered, seed=3):
    o, d = B.hand_rays(N)
    g = torch.Generator().manual_seed(seed + N)
    jit = torch.rand(N, generator=g) * (B.FAR - B.NEAR) / Sc if jittered else None
    zc, zf = torch.linspace(B.NEAR, B.FAR, Sc), torch.linspace(B.NEAR, B.FAR, Sf) if Sf else None
    return o, d, jit, zc, zf


@pytest.mark.parametrize("jittered", [True, False])
@pytest.mark.parametrize("Sc, Sf", [(3, 0), (64, 128), (65, 130)])
def test_ray_depths_equal_the_restatement_bit_for_bit(gpu_device, Sc, Sf, jittered):
    ops, dev = _ops(), gpu_device
    on = lambda t: None if t is None else t.to(dev).contiguous()
    for N in (0, 1, 63, 64, 65, 257):
        o, d, jit, zc, zf = _depths_case(N, Sc, Sf, jittered)
        z_c, z_f, span = ops.ray_depths(on(o), on(d), B.BOX, B.NEAR, B.FAR, on(jit), on(zc), on(zf))
        torch.cuda.synchronize()
        assert z_c.shape == (N, Sc) and span.shape == (N, 2) and ((z_f is None) if Sf == 0 else z_f.shape == (N, Sf))
        if N == 0:
            continue
        r_c, r_span, clipped = B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, jit, zc)
        assert same_bits(z_c, r_c), (N, int((bits(z_c) != bits(r_c)).sum()))
        assert same_bits(span, r_span)
        if Sf:
            assert same_bits(z_f, B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, jit, zf)[0])
        if N >= len(B.HAND):
            assert clipped[:len(B.HAND)].tolist() == [h[2] for h in B.HAND] and bool(clipped[len(B.HAND):].any()) and bool((~clipped[len(B.HAND):]).any())
        # what the restatement's properties (tests/test_ray_bounds_cpu.py) then say of the device's rows
        zc_h = z_c.cpu()
        assert bool((zc_h[:, 1:] >= zc_h[:, :-1]).all())
        today = zc.unsqueeze(0).expand(N, -1) + (0.0 if jit is None else jit.unsqueeze(1))
        assert torch.equal(bits(zc_h[~clipped]), bits(today[~clipped]))
        # against fp64: the bound is derived from the roundings (tests/ray_bounds_ref.py::affine_bound), it is not a measured number
        bound = B.affine_bound(B.FAR, (B.FAR - B.NEAR) / Sc if jittered else 0.0)
        assert float((zc_h - B.depths_exact(span.cpu(), B.NEAR, B.FAR, jit, zc)).abs().max()) <= bound
        if Sf:
            assert float((z_f.cpu() - B.depths_exact(span.cpu(), B.NEAR, B.FAR, jit, zf)).abs().max()) <= bound
    # without the span, and a box that clips nothing: today's rows
    z_c2, _, none = ops.ray_depths(on(o), on(d), B.BOX, B.NEAR, B.FAR, on(jit), on(zc), want_span=False)
    assert none is None and torch.equal(z_c2, z_c)
    z_all, _, span_all = ops.ray_depths(on(o), on(d), B.NO_CLIP, B.NEAR, B.FAR, on(jit), on(zc))
    finite = torch.isfinite(o).all(-1) & torch.isfinite(d).all(-1)
    assert same_bits(z_all, today) and bool((span_all.cpu() == torch.tensor([B.NEAR, B.FAR])).all()) and bool(finite.any())


def test_ray_depths_write_nothing_beyond_their_rows(gpu_device):
    """N = 65 rays (a part-filled workgroup) into buffers with guard words behind them: the library is called directly."""
    from mc_nerf_amd import _box
    ops, dev, N, Sc, Sf = _ops(), gpu_device, 65, 65, 130
    o, d, jit, zc, zf = _depths_case(N, Sc, Sf, True)
    on = lambda t: t.to(dev).contiguous()
    bufs = [torch.full((n + 64,), -7.0, device=dev) for n in (N * Sc, N * Sf, N * 2)]
    _box.call("mcnerf_box_ray_depths", on(o), on(d), N, *B.BOX, B.NEAR, B.FAR, on(jit), on(zc), Sc, on(zf), Sf, *bufs, ops._stream())
    torch.cuda.synchronize()
    for buf, n, grid in zip(bufs[:2], (N * Sc, N * Sf), (zc, zf)):
        assert bool((buf[n:] == -7.0).all())
        assert same_bits(buf[:n].view(N, -1), B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, jit, grid)[0])
    assert bool((bufs[2][2 * N:] == -7.0).all())


# ------------------------------------------------------------------------------------------------------ 2. sample_pdf on rows
@pytest.mark.parametrize("Sc, I", [(3, 1), (64, 128), (65, 64), (512, 512)])
def test_sample_pdf_rows_equal_the_grid_entry_point_on_its_own_depths(gpu_device, Sc, I):
    ops, dev, N = _ops(), gpu_device, 257
    g = torch.Generator().manual_seed(Sc * 7 + I)
    zgrid = torch.linspace(B.NEAR, B.FAR, Sc)
    jit = torch.rand(N, generator=g) * (B.FAR - B.NEAR) / Sc
    w, u = torch.rand(N, Sc, generator=g), torch.rand(N, I, generator=g)
    w[5], w[6, Sc // 2] = 0.0, 50.0
    rows = (zgrid.unsqueeze(0) + jit.unsqueeze(1)).contiguous()
    on = lambda t: t.to(dev).contiguous()
    for jitter, r in ((jit, rows), (None, zgrid.unsqueeze(0).expand(N, -1).contiguous())):
        want = ops.sample_pdf(on(w), on(zgrid), None if jitter is None else on(jitter), on(u))
        out = torch.full((N + 2, Sc + I), float("nan"), device=dev)
        got = ops.sample_pdf(on(w), None, None, on(u), out=out[1:N + 1], z_rows=on(r))
        torch.cuda.synchronize()
        assert same_bits(got, want) and not bool(torch.isnan(got).any())
        assert bool(torch.isnan(out[0]).all()) and bool(torch.isnan(out[N + 1]).all())
    assert ops.sample_pdf(on(w[:0]), None, None, on(u[:0]), z_rows=on(rows[:0])).shape == (0, Sc + I)


def test_sample_pdf_rows_match_the_restatement_on_clipped_rows(gpu_device):
    """Rows from ray_depths on the hand-made rays (clipped spans down to a fraction of a unit, unclipped ones, NaN rays left out: their
    rows are today's).  Held to `check_rows` of tests/test_pdf_sampler_gpu.py::test_sampler_kernel_matches_the_restatement, criterion by
    criterion -- sorted, the coarse depths bit for bit, every importance sample inside the restatement's u -+ 1e-6 bracket, 99.9 % of
    them within 2e-6 of the restatement's -- with tests/pdf_ref.py called ray by ray, which takes each ray's own row as its grid."""
    ops, dev, N, Sc, I = _ops(), gpu_device, 257, 64, 128
    o, d, jit, zc, _ = _depths_case(N, Sc, 0, True)
    on = lambda t: t.to(dev).contiguous()
    rows_d, _, span = ops.ray_depths(on(o), on(d), B.BOX, B.NEAR, B.FAR, on(jit), on(zc))
    rows = rows_d.cpu()
    assert same_bits(rows, B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, jit, zc)[0])
    g = torch.Generator().manual_seed(17)
    w, u = torch.rand(N, Sc, generator=g) ** 4, torch.rand(N, I, generator=g)
    z_all = ops.sample_pdf(on(w), None, None, on(u), z_rows=rows_d).cpu()
    assert bool((z_all[:, 1:] >= z_all[:, :-1]).all()), "z_all is not sorted"
    _, zs_ref, zc_ref = B.sample_pdf_rows_ref(w, rows, u)
    zs_dev, zc_found = split_rows(z_all, zc_ref)
    assert same_bits(zc_found, rows), "the coarse depths are not in z_all bit for bit"
    du = 1e-6
    lo = torch.sort(B.sample_pdf_rows_ref(w, rows, u - du)[1], 1).values
    hi = torch.sort(B.sample_pdf_rows_ref(w, rows, u + du)[1], 1).values
    out = ~((zs_dev >= lo) & (zs_dev <= hi))
    assert not bool(out.any()), f"{int(out.sum())} importance samples outside the u +- {du} bracket"
    close = float(((zs_dev - torch.sort(zs_ref, 1).values).abs() <= 2e-6).float().mean())
    assert close >= 0.999, close
    clipped = (span[:, 1] - span[:, 0]).cpu() < (B.FAR - B.NEAR)
    inside = (zs_dev >= rows[:, :1]) & (zs_dev <= rows[:, -1:])
    assert bool(clipped.any()) and bool(inside[clipped].all())           # the importance samples of a clipped ray stay inside its span


# ---------------------------------------------------------------------------------------------------- 3. voxel select / update
def _sigma(N, Sc, g):
    """Eight levels, so the per-cell maxima tie, with a NaN and two infinities mixed in (tests/test_voxel_gpu.py::_quantised_sigma)."""
    sig = (torch.randint(0, 8, (N, Sc), generator=g).float() - 4.0) * 0.5
    bad = torch.randperm(N * Sc, generator=g)[:3]
    sig.view(-1)[bad] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    return torch.cat([sig.unsqueeze(-1), torch.rand(N, Sc, 3, generator=g)], -1).contiguous()


def _grid(ops, vox, dev):
    grid = ops.VoxelGrid(vox.shape[0], BMIN, BMAX, SIGMA_INIT, dev)
    grid.vox.copy_(vox.to(dev))
    return grid


@pytest.mark.parametrize("N, Sc", [(15, 17), (4, 64), (257, 1)])           # N Sc = 255, 256, 257
@pytest.mark.parametrize("G", [2, 17])
def test_voxel_rows_entry_points(gpu_device, G, N, Sc):
    ops, dev = _ops(), gpu_device
    on = lambda t: t.to(dev).contiguous()
    o, d, jit, zc, _ = _depths_case(N, Sc, 0, True)
    g = torch.Generator().manual_seed(G * 100 + N)
    vox0 = torch.rand(G, G, G, generator=g) * 2.0 - 1.0
    sig = _sigma(N, Sc, g)

    def device(rows, jitter, listed):
        """select + two updates (dense, then on the list or on all pairs) with the depths as rows, or as grid + jitter."""
        zg, jt, kw = (on(zc), on(jitter), {}) if rows is None else (None, None, dict(z_rows=on(rows)))
        grid = _grid(ops, vox0, dev)
        sentinel = torch.full((N * Sc, 2), -7, dtype=torch.int32, device=dev)
        idx, count, out_c = ops.voxel_select(grid, 0.0, on(o), on(d), zg, jt, SIGMA_DEFAULT, idx=sentinel, **kw)
        k = int(count.item())
        ops.voxel_update(grid, 0.25, on(o), on(d), zg, jt, on(sig), **kw)
        v1 = grid.vox.clone()
        if listed:
            ops.voxel_update(grid, 1.0, on(o), on(d), zg, jt, on(sig), idx, count, N * Sc, **kw)
        torch.cuda.synchronize()
        assert int(grid.scratch.count_nonzero()) == 0
        return idx.cpu(), k, out_c.cpu(), v1.cpu(), grid.vox.cpu()

    # ---- the identity: rows fl(zgrid + jitter) against the grid entry points
    today = (zc.unsqueeze(0) + jit.unsqueeze(1)).contiguous()
    a, b = device(None, jit, True), device(today, None, True)
    assert a[1] == b[1] and torch.equal(a[0], b[0]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3]) and same_bits(a[4], b[4])
    assert bool((b[0][b[1]:] == -7).all())
    # ---- clipped rows (the device's own, which test 1 holds to the restatement) against the torch restatement
    rows = ops.ray_depths(on(o), on(d), B.BOX, B.NEAR, B.FAR, on(jit), on(zc))[0].cpu()
    assert same_bits(rows, B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, jit, zc)[0])
    idx, k, out_c, v1, v2 = device(rows, None, True)
    ref_idx, ref_out = B.select_rows(vox0, 0.0, o, d, rows, BMIN, BMAX, SIGMA_DEFAULT)
    assert k == ref_idx.shape[0] and torch.equal(idx[:k].long(), ref_idx) and bool((idx[k:] == -7).all()) and same_bits(out_c, ref_out)
    assert 0 < k < N * Sc
    r1 = B.update_rows(vox0, 0.25, o, d, rows, sig[..., 0], BMIN, BMAX)
    assert same_bits(v1, r1)
    assert same_bits(v2, B.update_rows(r1, 1.0, o, d, rows, sig[..., 0], BMIN, BMAX, ref_idx))
    cells = B.cells_rows(o, d, rows, G, BMIN, BMAX)
    touched = torch.zeros(G ** 3, dtype=torch.bool)
    touched[cells.reshape(-1)[torch.isfinite(sig[..., 0].reshape(-1))]] = True
    assert same_bits(v1.reshape(-1)[~touched], vox0.reshape(-1)[~touched])
