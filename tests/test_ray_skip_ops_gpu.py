"""The hit library's entry points (include/mcnerf_hit.h; csrc/ray_skip.hip) on the GPU.  Every list comparison is integer and exact.

  1. ray_depths with hit   z_c, z_f and span are mcnerf_box_ray_depths' bits, hit is the restatement's flag (tests/ray_skip_ref.py), on the
                           hand-made rays at every size of the bounds library's own test;
  2. list_rays             idx[:count], count and the prefill against the restatement: all rays, none (count == 0, idx untouched), the
                           hand-made rays' flags; nothing is written beyond the buffers;
  3. select_fine(hit=)     with all ones mcnerf_select_fine's list, count and prefill bit for bit; with a mask that list filtered by ray,
                           in order; a threshold above every weight (the maximum decides); NaN weights in a masked ray;
  4. voxel_select(hit=)    the same pair of statements against voxel_select(z_rows=) on clipped rows;
  5. the listed MLP pass   mlp_fwd on list_rays' list over per-ray rows, all five precision modes: a masked ray's rows keep the prefill's
                           bits, a hit ray's are those of the same call with every ray listed.
"""
import pytest
import torch

import ray_bounds_ref as B
import ray_skip_ref as R
from test_pdf_sampler_gpu import MODES, SIZES
from test_voxel_gpu import _voxel_model

pytestmark = pytest.mark.gpu
BMIN, BMAX, SIGMA_INIT, SIGMA_DEFAULT = -3.5, 3.5, 30.0, -20.0


def _ops():
    from mc_nerf_amd import ops
    return ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _hand_hit(N):
    o, d = B.hand_rays(N)
    return o, d, R.hit_ref(o, d, B.BOX, B.NEAR, B.FAR)


def _masks(N):
    """all-hit, none-hit and the hand-made rays' flags (with values other than 1 among the non-zero ones: the predicate is != 0)."""
    hand = _hand_hit(N)[2]
    hand = torch.where(hand != 0, torch.arange(N, dtype=torch.int32) % 3 - 3, hand)        # -3, -2, -1 on the hits
    return dict(all=torch.ones(N, dtype=torch.int32), none=torch.zeros(N, dtype=torch.int32), hand=hand)


# --------------------------------------------------------------------------------------------------------- 1. ray_depths with hit
@pytest.mark.parametrize("jittered", [True, False])
@pytest.mark.parametrize("Sc, Sf", [(3, 0), (64, 128), (65, 130)])
def test_ray_depths_with_hit_are_the_box_entry_points_bits_and_the_restated_flag(gpu_device, Sc, Sf, jittered):
    ops, dev = _ops(), gpu_device
    on = lambda t: None if t is None else t.to(dev).contiguous()
    for N in (0, 1, 63, 64, 65, 257):
        o, d, want_hit = _hand_hit(N)
        g = torch.Generator().manual_seed(3 + N)
        jit = torch.rand(N, generator=g) * (B.FAR - B.NEAR) / Sc if jittered else None
        zc, zf = torch.linspace(B.NEAR, B.FAR, Sc), torch.linspace(B.NEAR, B.FAR, Sf) if Sf else None
        args = (on(o), on(d), B.BOX, B.NEAR, B.FAR, on(jit), on(zc), on(zf))
        b_c, b_f, b_span = ops.ray_depths(*args)
        z_c, z_f, span, hit = ops.ray_depths(*args, want_hit=True)
        torch.cuda.synchronize()
        assert hit.shape == (N,) and hit.dtype == torch.int32
        assert same_bits(z_c, b_c) and same_bits(span, b_span) and ((z_f is None and b_f is None) if Sf == 0 else same_bits(z_f, b_f))
        assert torch.equal(hit.cpu(), want_hit), N
        if N >= len(B.HAND):
            assert hit.cpu()[:len(B.HAND)].tolist() == [int(h[2]) for h in B.HAND]
        if N == 257:
            assert int(hit.sum()) == 116
            no_span = ops.ray_depths(*args, want_span=False, want_hit=True)
            assert no_span[2] is None and torch.equal(no_span[3], hit) and same_bits(no_span[0], b_c)


def test_ray_depths_with_hit_write_nothing_beyond_their_rows(gpu_device):
    """N = 65 rays (a part-filled workgroup) into buffers with guard words behind them: the library is called directly."""
    from mc_nerf_amd import _hit
    ops, dev, N, Sc, Sf = _ops(), gpu_device, 65, 65, 130
    o, d, want_hit = _hand_hit(N)
    on = lambda t: t.to(dev).contiguous()
    zc, zf = torch.linspace(B.NEAR, B.FAR, Sc), torch.linspace(B.NEAR, B.FAR, Sf)
    bufs = [torch.full((n + 64,), -7.0, device=dev) for n in (N * Sc, N * Sf, N * 2)]
    hit = torch.full((N + 64,), -7, dtype=torch.int32, device=dev)
    _hit.call("mcnerf_hit_ray_depths", on(o), on(d), N, *B.BOX, B.NEAR, B.FAR, None, on(zc), Sc, on(zf), Sf, *bufs, hit, ops._stream())
    torch.cuda.synchronize()
    for buf, n in zip(bufs, (N * Sc, N * Sf, N * 2)):
        assert bool((buf[n:] == -7.0).all())
    assert bool((hit[N:] == -7).all()) and torch.equal(hit[:N].cpu(), want_hit)
    assert same_bits(bufs[0][:N * Sc].view(N, Sc), B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, None, zc)[0])


# ------------------------------------------------------------------------------------------------------------------ 2. list_rays
@pytest.mark.parametrize("S", [3, 64, 65, 130])
@pytest.mark.parametrize("mask", ["all", "none", "hand"])
def test_list_rays_equals_the_restatement(gpu_device, S, mask):
    ops, dev, N = _ops(), gpu_device, 257
    hit = _masks(N)[mask]
    ref_idx, ref_out = R.list_rays_ref(hit, S, SIGMA_DEFAULT)
    sentinel = torch.full((N * S + 8, 2), -7, dtype=torch.int32, device=dev)
    idx, count, out = ops.list_rays(hit.to(dev), S, SIGMA_DEFAULT, idx=sentinel)
    torch.cuda.synchronize()
    k = int(count.item())
    assert idx is sentinel and k == ref_idx.shape[0] == S * int((hit != 0).sum())
    assert torch.equal(idx[:k].cpu().long(), ref_idx) and bool((idx[k:] == -7).all())                # (k == 0: idx untouched)
    assert same_bits(out, ref_out)
    if mask == "all":
        every = torch.stack(torch.meshgrid(torch.arange(N), torch.arange(S), indexing="ij"), -1).reshape(-1, 2)
        assert torch.equal(idx[:k].cpu().long(), every)
    # without the prefill and into its own buffer: the same list; two runs give the same list
    idx2, count2, none = ops.list_rays(hit.to(dev), S, SIGMA_DEFAULT, prefill=False)
    assert none is None and int(count2.item()) == k and torch.equal(idx2[:k], idx[:k]) and idx2.shape == (N * S, 2)
    # no rays at all
    idx0, _, out0 = ops.list_rays(hit[:0].to(dev), S, SIGMA_DEFAULT)
    assert idx0.shape == (0, 2) and out0.shape == (0, S, 4)


@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_list_rays_at_the_edges_of_a_workgroup(gpu_device, N):
    ops, dev, S = _ops(), gpu_device, 65
    hit = _masks(N)["hand"]
    ref_idx, ref_out = R.list_rays_ref(hit, S, SIGMA_DEFAULT)
    out = torch.full((N * S * 4 + 64,), -7.0, device=dev)
    idx, count, rc, ro, _ = ops._list_buffers(N, S, False, torch.full((N * S + 8, 2), -7, dtype=torch.int32, device=dev), dev)
    from mc_nerf_amd import _hit
    _hit.call("mcnerf_hit_list_rays", hit.to(dev), N, S, SIGMA_DEFAULT, rc, ro, idx, count, out, ops._stream())
    torch.cuda.synchronize()
    k = int(count.item())
    assert k == ref_idx.shape[0] and torch.equal(idx[:k].cpu().long(), ref_idx) and bool((idx[k:] == -7).all())
    assert same_bits(out[:N * S * 4].view(N, S, 4), ref_out) and bool((out[N * S * 4:] == -7.0).all())
    assert torch.equal(rc.cpu(), (hit != 0).to(torch.int32) * S)


# ------------------------------------------------------------------------------------------------------------ 3. select_fine(hit=)
def _weights(N, Sc, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(N, Sc, generator=g) ** 6                      # a few per cent of them above 0.5
    return w, w.max().reshape(1).view(torch.int32)


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("Sc", [32, 65])
@pytest.mark.parametrize("case", ["threshold", "wmax decides", "nan in a masked ray"])
def test_select_fine_behind_the_flag(gpu_device, case, Sc, scale):
    ops, dev, N = _ops(), gpu_device, 257
    on = lambda t: t.to(dev).contiguous()
    w, wmax = _weights(N, Sc, 7 * Sc + scale)
    thresh = 2.0 if case == "wmax decides" else 0.5              # 2.0: every weight is below it, min(thresh, wmax) = wmax
    masks = _masks(N)
    ones, hand = masks["all"], masks["hand"]
    if case == "wmax decides":                                   # the maximum sits in two hit rays and in one masked ray
        n_hit, n_miss = (hand != 0).nonzero().reshape(-1), (hand == 0).nonzero().reshape(-1)
        w[n_hit[3], 5] = w[n_hit[40], Sc - 1] = w[n_miss[2], 7] = 1.5
        wmax = w.max().reshape(1).view(torch.int32)
    plain = ops.select_fine(on(w), on(wmax), thresh, scale, SIGMA_DEFAULT)
    k0 = int(plain[1].item())
    assert 0 < k0 < N * Sc * scale
    # ---- all ones: the core entry point's list, count and prefill bit for bit
    idx, count, out_f = ops.select_fine(on(w), on(wmax), thresh, scale, SIGMA_DEFAULT, hit=on(ones))
    torch.cuda.synchronize()
    assert int(count.item()) == k0 and torch.equal(idx[:k0], plain[0][:k0]) and same_bits(out_f, plain[2])
    # ---- a mask: that list filtered by ray, in order (and the restatement's)
    w_in = w
    if case == "nan in a masked ray":
        w_in = w.clone()
        w_in[hand == 0] = float("nan")                           # never read: the list is that of the clean weights
    idx, count, out_f = ops.select_fine(on(w_in), on(wmax), thresh, scale, SIGMA_DEFAULT, hit=on(hand))
    torch.cuda.synchronize()
    k = int(count.item())
    want = R.filter_by_ray(plain[0][:k0].cpu().long(), hand)
    assert k == want.shape[0] and torch.equal(idx[:k].cpu().long(), want) and same_bits(out_f, plain[2])
    assert torch.equal(want, R.select_fine_ref(w, w.max(), thresh, scale, SIGMA_DEFAULT, hand)[0])
    assert torch.equal(want, R.oracle_select_on_hits(w, thresh, scale, hand))
    assert 0 < k < k0
    if case == "wmax decides":
        assert (k0, k) == (3 * scale, 2 * scale)
    # ---- no ray hits: an empty list over the full prefill, without the prefill too
    idx, count, out_f = ops.select_fine(on(w), on(wmax), thresh, scale, SIGMA_DEFAULT, hit=on(masks["none"]))
    assert int(count.item()) == 0 and same_bits(out_f, plain[2])
    assert ops.select_fine(on(w), on(wmax), thresh, scale, SIGMA_DEFAULT, prefill=False, hit=on(hand))[2] is None


# ----------------------------------------------------------------------------------------------------------- 4. voxel_select(hit=)
@pytest.mark.parametrize("N, Sc", [(257, 32), (65, 65)])
def test_voxel_select_behind_the_flag(gpu_device, N, Sc):
    ops, dev, G = _ops(), gpu_device, 16
    on = lambda t: t.to(dev).contiguous()
    o, d, hit = _hand_hit(N)
    g = torch.Generator().manual_seed(N + Sc)
    jit = torch.rand(N, generator=g) * (B.FAR - B.NEAR) / Sc
    zc = torch.linspace(B.NEAR, B.FAR, Sc)
    vox0 = torch.rand(G, G, G, generator=g) * 2.0 - 1.0
    grid = ops.VoxelGrid(G, BMIN, BMAX, SIGMA_INIT, dev)
    grid.vox.copy_(vox0.to(dev))
    rows_d, _, _, hit_d = ops.ray_depths(on(o), on(d), B.BOX, B.NEAR, B.FAR, on(jit), on(zc), want_hit=True)
    assert torch.equal(hit_d.cpu(), hit)
    plain = ops.voxel_select(grid, 0.0, on(o), on(d), None, None, SIGMA_DEFAULT, z_rows=rows_d)
    k0 = int(plain[1].item())
    assert 0 < k0 < N * Sc
    # ---- all ones: the bounds library's list, count and prefill
    ones = torch.ones(N, dtype=torch.int32, device=dev)
    idx, count, out_c = ops.voxel_select(grid, 0.0, on(o), on(d), None, None, SIGMA_DEFAULT, z_rows=rows_d, hit=ones)
    torch.cuda.synchronize()
    assert int(count.item()) == k0 and torch.equal(idx[:k0], plain[0][:k0]) and same_bits(out_c, plain[2])
    # ---- the rays' own flags: that list filtered by ray, in order, which is the restatement's
    sentinel = torch.full((N * Sc, 2), -7, dtype=torch.int32, device=dev)
    idx, count, out_c = ops.voxel_select(grid, 0.0, on(o), on(d), None, None, SIGMA_DEFAULT, idx=sentinel, z_rows=rows_d, hit=hit_d)
    torch.cuda.synchronize()
    k = int(count.item())
    want = R.filter_by_ray(plain[0][:k0].cpu().long(), hit)
    ref_idx, ref_out = R.voxel_select_ref(vox0, 0.0, o, d, rows_d.cpu(), BMIN, BMAX, SIGMA_DEFAULT, hit)
    assert k == want.shape[0] and torch.equal(idx[:k].cpu().long(), want) and torch.equal(want, ref_idx) and bool((idx[k:] == -7).all())
    assert same_bits(out_c, ref_out) and 0 < k < k0
    # ---- NaN and inf rays are masked: a grid of NaN-free cells is never indexed by their samples (the list names none of them)
    assert not bool(torch.isin(idx[:k, 0].cpu().long(), (hit == 0).nonzero().reshape(-1)).any())
    none = ops.voxel_select(grid, 0.0, on(o), on(d), None, None, SIGMA_DEFAULT, z_rows=rows_d, hit=torch.zeros_like(ones))
    assert int(none[1].item()) == 0 and same_bits(none[2], plain[2])


# ----------------------------------------------------------------------------------------------------------- 5. the listed MLP pass
@pytest.mark.parametrize("precision", MODES)
def test_listed_mlp_pass_leaves_masked_rays_at_the_prefill(gpu_device, precision):
    ops, dev, N, S = _ops(), gpu_device, 257, 32
    assert SIZES["small"][0] == S
    m, _, _, _ = _voxel_model(dev, precision, N)
    on = lambda t: t.to(dev).contiguous()
    o, d, hit = _hand_hit(N)
    finite = torch.isfinite(o).all(-1) & torch.isfinite(d).all(-1)
    o, d = torch.where(finite.unsqueeze(1), o, torch.zeros_like(o)), torch.where(finite.unsqueeze(1), d, torch.ones_like(d))    # (every ray is evaluated in the all-ones call)
    g = torch.Generator().manual_seed(9)
    jit = torch.rand(N, generator=g) * (B.FAR - B.NEAR) / S
    rows, _, _, _ = ops.ray_depths(on(o), on(d), B.BOX, B.NEAR, B.FAR, on(jit), m.z_vals_c, want_hit=True)
    model = m.nerf_coarse
    flat = model.flat_params()
    packed = ops.pack_weights(model.net, flat, precision=precision)
    barf = m.emmbedding_xyz.barf_weights_on(1.0, dev, pad=10)
    outs = {}
    for name, h in (("all", torch.ones(N, dtype=torch.int32)), ("hand", hit)):
        idx, count, out = ops.list_rays(on(h), S, SIGMA_DEFAULT)
        ops.mlp_fwd(model.net, flat, packed, on(o), on(d), None, None, barf, out, idx=idx, count=count, max_rows=N * S, precision=precision, z_rows=rows)
        torch.cuda.synchronize()
        outs[name] = out.cpu()
    prefill = R.prefill_ref(N, S, SIGMA_DEFAULT)
    masked = hit == 0
    assert 0 < int(masked.sum()) < N
    assert same_bits(outs["hand"][masked], prefill[masked])
    assert same_bits(outs["hand"][~masked], outs["all"][~masked])
    assert not bool((bits(outs["all"]) == bits(prefill)).all(-1).all(-1).any())          # ... every ray of which was evaluated
