"""The fit library's entry points (include/mcnerf_fit.h; csrc/scene_fit.hip) on the GPU.  Every comparison is equality.

  1. voxel_box    cells and box against the torch-CPU restatement (tests/scene_fit_ref.py), bit for bit, and a second run against the
                  first: grid sizes below, at and above a wave's and a workgroup's stride and one whose grid-stride loop wraps; no, every
                  and single occupied cells, cells at the threshold, NaN and both infinities; every margin; outer boxes that cut the fit
                  and that lie beside it; a grid that does not start on a 16-byte boundary;
  2. ray_depths   with the box on the device against the same call with the six values as a tuple (the existing kernel) and against
                  tests/ray_bounds_ref.py, bit for bit; and fed by voxel_box with no host copy in between.
"""
import pytest
import torch

import ray_bounds_ref as B
import scene_fit_ref as F

pytestmark = pytest.mark.gpu
BMIN, BMAX = -3.5, 3.5
CUBE = (BMIN,) * 3 + (BMAX,) * 3
SIZES = (2, 3, 5, 64, 65, 130)          # 8 cells .. 2.2 M: below a wave, a workgroup and the 2048-workgroup stride, and (130) above it
MARGINS = lambda G: (0, 1, 2, G)
NAN, INF = float("nan"), float("inf")


def _ops():
    from mc_nerf_amd import ops
    return ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _grid(dev, vox, offset=0):
    """An ops.VoxelGrid over CUBE holding `vox`; `offset` floats off a fresh allocation's 16-byte boundary."""
    ops, G = _ops(), vox.shape[0]
    grid = ops.VoxelGrid(G, BMIN, BMAX, 0.0, dev)
    if offset:
        buf = torch.empty(G ** 3 + offset, dtype=torch.float32, device=dev)
        grid.vox = buf[offset:].view(G, G, G)
        assert grid.vox.data_ptr() % 16 == 4 * offset and grid.vox.is_contiguous()
    grid.vox.copy_(vox)
    assert grid.h == F.cell_edge(G, BMIN, BMAX)
    return grid


def _fit_equals_the_restatement(grid, vox, thresh, margin, outer):
    ops = _ops()
    cells, box = ops.voxel_box(grid, thresh, margin, outer)
    again = ops.voxel_box(grid, thresh, margin, outer, torch.full_like(cells, 77), torch.full_like(box, 77.0))
    r_cells, r_box = F.voxel_box_ref(vox, grid.bmin, grid.h, thresh, margin, outer)
    assert cells.dtype == torch.int32 and box.dtype == torch.float32 and cells.shape == (8,) and box.shape == (6,)
    assert torch.equal(cells.cpu(), r_cells), (cells.tolist(), r_cells.tolist(), margin)
    assert same_bits(box, r_box), (box.tolist(), r_box.tolist(), margin)
    assert torch.equal(again[0], cells) and same_bits(again[1], box)             # ... and a second run gives identical bits
    return r_cells, r_box


def _grids(G, kind):
    """-> [(vox, thresh)] of one kind."""
    if kind == "empty":
        return [(F.grid_with(G, []), 0.0)]
    if kind == "full":
        return [(F.grid_with(G, [], below=1.0), 0.0)]
    if kind == "single":                                                        # each corner, and one cell inside (G = 2 has no inside)
        cells = F.corners(G) + [(G // 2, max(G // 3, 0), G - 1 - G // 4)]
        return [(F.grid_with(G, [c]), 0.0) for c in cells]
    if kind == "opposite":
        return [(F.grid_with(G, [a, tuple(G - 1 - v for v in a)]), 0.0) for a in F.corners(G)[:4]]
    if kind == "random":
        return [(F.random_fill(G, 0.01, 100 + G), 0.0)]
    if kind == "special":                                                       # only the +inf cell is occupied; then nothing is
        t = 0.25
        c = [(0, 0, G - 1, t), (G - 1, 0, 0, NAN), (G - 1, G - 1, 0, -INF), (1, G - 1, 1, INF)]
        return [(F.grid_with(G, c, below=-1.0), t), (F.grid_with(G, c[:3], below=-1.0), t), (torch.full((G, G, G), NAN), t),
                (F.grid_with(G, [(0, 1, 0, 1.0)], below=NAN), t)]
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------- 1. voxel_box
@pytest.mark.parametrize("kind", ["empty", "full", "single", "opposite", "random", "special"])
@pytest.mark.parametrize("G", SIZES)
def test_voxel_box_equals_the_restatement(gpu_device, G, kind):
    dev = gpu_device
    seen = set()
    for vox, thresh in _grids(G, kind):
        grid = _grid(dev, vox)
        for margin in MARGINS(G):
            r_cells, r_box = _fit_equals_the_restatement(grid, vox, thresh, margin, CUBE)
            seen.add(int(r_cells[6]))
            if margin == G and int(r_cells[6]) == 1:                            # a margin of G pads to the whole cube
                assert r_box.tolist() == list(CUBE)
    assert seen == ({0} if kind == "empty" else {1} if kind in ("full", "single", "opposite") else {0, 1} if kind == "special" else seen)
    if kind == "random" and G >= 64:
        assert seen == {1}


def test_the_grid_stride_loop_wraps(gpu_device):
    """G = 160: 1 024 000 float4s, 4000 workgroups' worth for the 2048 there are.  Single cells at both ends of the grid and of the second
    sweep, then a 1 % fill."""
    dev, G = gpu_device, 160
    second = 2048 * 256 * 4                                                     # the first cell of thread 0's second float4
    at = lambda i: (i // (G * G), (i // G) % G, i % G)
    vox = F.grid_with(G, [])
    grid = _grid(dev, vox)
    for cells in ([at(second)], [at(second - 1)], [at(G ** 3 - 1)], [at(second + 5), at(G ** 3 - 2)], [at(0), at(second + G * G)]):
        for c in cells:
            vox[c] = 1.0
        grid.vox.copy_(vox)
        r_cells, _ = _fit_equals_the_restatement(grid, vox, 0.0, 1, CUBE)
        assert r_cells.tolist()[:3] == [min(c[k] for c in cells) for k in range(3)]
        for c in cells:
            vox[c] = -1.0
    vox = F.random_fill(G, 0.01, 7)
    grid.vox.copy_(vox)
    for margin in (0, 2):
        _fit_equals_the_restatement(grid, vox, 0.0, margin, CUBE)


@pytest.mark.parametrize("G", [5, 65])
def test_a_grid_off_the_16_byte_boundary(gpu_device, G):
    """The cells in front of the first boundary and behind the last whole float4 are read one by one: single cells there, and a fill."""
    dev = gpu_device
    for offset in (1, 2, 3):
        lead = 4 - offset
        ends = [0, lead - 1, lead, G ** 3 - 1, G ** 3 - 2, G ** 3 - 4]
        at = lambda i: (i // (G * G), (i // G) % G, i % G)
        for vox in [F.grid_with(G, [at(i)]) for i in ends] + [F.random_fill(G, 0.05, offset)]:
            _fit_equals_the_restatement(_grid(dev, vox, offset), vox, 0.0, 1, CUBE)


@pytest.mark.parametrize("thresh", [-0.99, 0.99])
@pytest.mark.parametrize("G", [5, 64, 65])
def test_negative_and_positive_thresholds(gpu_device, G, thresh):
    g = torch.Generator().manual_seed(G)
    vox = torch.rand(G, G, G, generator=g) * 2.0 - 1.0
    if thresh < 0:                                                              # occupied is then the rule: empty all but ~1 %
        vox = torch.where(torch.rand(G, G, G, generator=g) < 0.01, vox, torch.tensor(-1.0))
    grid = _grid(gpu_device, vox)
    for margin in (0, 2):
        _fit_equals_the_restatement(grid, vox, thresh, margin, CUBE)
    assert G < 64 or 0 < int((vox > thresh).sum()) < G ** 3 // 10


@pytest.mark.parametrize("G", [5, 64])
def test_outer_boxes_that_cut_the_fit_and_that_miss_it(gpu_device, G):
    vox = F.blob(G, (G // 4,) * 3, (G // 2, G // 2 + 1, G - 2))
    grid = _grid(gpu_device, vox)
    for margin in (0, 1, G):
        _, fit = _fit_equals_the_restatement(grid, vox, 0.0, margin, CUBE)
        lo, hi = fit[:3].tolist(), fit[3:].tolist()
        mid = [(a + b) / 2 for a, b in zip(lo, hi)]
        cut = (mid[0], lo[1] - 1.0, lo[2], hi[0] + 1.0, mid[1], hi[2])          # cuts x from below and y from above
        cells, box = _fit_equals_the_restatement(grid, vox, 0.0, margin, cut)
        assert int(cells[6]) == 1 and float(box[0]) == float(torch.tensor(mid[0])) and float(box[4]) == float(torch.tensor(mid[1]))
        for beside in ((hi[0], lo[1], lo[2], hi[0] + 1.0, hi[1], hi[2]),        # touches the fit in x: lo == hi
                       (20.0, 20.0, 20.0, 21.0, 21.0, 21.0)):
            cells, box = _fit_equals_the_restatement(grid, vox, 0.0, margin, beside)
            assert int(cells[6]) == 2 and box.tolist() == [float(torch.tensor(v)) for v in beside]
            assert cells.tolist()[:6] == [G // 4] * 3 + [G // 2, G // 2 + 1, G - 2]


# --------------------------------------------------------------------------------------------------------------- 2. ray_depths
def _depths_case(rays, N, Sc, Sf, jittered):
    if rays == "hand":
        o, d = B.hand_rays(N)
    else:
        d, o = B.model_rays(N)
    g = torch.Generator().manual_seed(3 + N)
    jit = torch.rand(N, generator=g) * (B.FAR - B.NEAR) / Sc if jittered else None
    return o, d, jit, torch.linspace(B.NEAR, B.FAR, Sc), torch.linspace(B.NEAR, B.FAR, Sf) if Sf else None


@pytest.mark.parametrize("jittered", [True, False])
@pytest.mark.parametrize("Sf", [0, 128, 130])
@pytest.mark.parametrize("Sc", [3, 64, 65])
@pytest.mark.parametrize("rays", ["hand", "model"])
def test_ray_depths_from_a_device_box_equal_the_tuple_form_and_the_restatement(gpu_device, rays, Sc, Sf, jittered):
    ops, dev = _ops(), gpu_device
    on = lambda t: None if t is None else t.to(dev).contiguous()
    box_d = torch.tensor(B.BOX, device=dev)
    for N in (1, 3, 257):
        o, d, jit, zc, zf = _depths_case(rays, N, Sc, Sf, jittered)
        args = (on(o), on(d))
        rest = (B.NEAR, B.FAR, on(jit), on(zc), on(zf))
        z_c, z_f, span, hit = ops.ray_depths(*args, box_d, *rest, want_hit=True)
        assert z_c.shape == (N, Sc) and span.shape == (N, 2) and hit.shape == (N,) and hit.dtype == torch.int32
        # the existing kernel on the same six values: the independent yardstick
        t_c, t_f, t_span, t_hit = ops.ray_depths(*args, B.BOX, *rest, want_hit=True)
        b_c, b_f, b_span = ops.ray_depths(*args, B.BOX, *rest)
        for got, want in ((z_c, t_c), (span, t_span), (z_c, b_c), (span, b_span)):
            assert same_bits(got, want)
        assert torch.equal(hit, t_hit) and ((z_f is None and t_f is None) if Sf == 0 else (same_bits(z_f, t_f) and same_bits(z_f, b_f)))
        # the restatement
        r_c, r_span, clipped = B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, jit, zc)
        assert same_bits(z_c, r_c) and same_bits(span, r_span) and torch.equal(hit.cpu(), clipped.to(torch.int32))
        if Sf:
            assert same_bits(z_f, B.depths_ref(o, d, B.BOX, B.NEAR, B.FAR, jit, zf)[0])
        if rays == "hand" and N >= len(B.HAND):
            assert clipped[:len(B.HAND)].tolist() == [h[2] for h in B.HAND]
        # without the flag, without the span, without either: the same rows
        for want_span, want_hit in ((True, False), (False, True), (False, False)):
            out = ops.ray_depths(*args, box_d, *rest, want_span=want_span, want_hit=want_hit)
            assert len(out) == (4 if want_hit else 3) and same_bits(out[0], z_c) and ((out[1] is None) if Sf == 0 else same_bits(out[1], z_f))
            assert (out[2] is None) if not want_span else same_bits(out[2], span)
            assert not want_hit or torch.equal(out[3], hit)
    # N = 0: nothing is read or written
    e = torch.zeros(0, 3, device=dev)
    z0, _, s0, h0 = ops.ray_depths(e, e, box_d, B.NEAR, B.FAR, None, on(zc), want_hit=True)
    assert z0.shape == (0, Sc) and s0.shape == (0, 2) and h0.shape == (0,)


def test_a_nan_box_clips_no_ray(gpu_device):
    ops, dev = _ops(), gpu_device
    o, d, jit, zc, _ = _depths_case("model", 64, 16, 0, True)
    z_c, _, span, hit = ops.ray_depths(o.to(dev), d.to(dev), torch.full((6,), NAN, device=dev), B.NEAR, B.FAR, jit.to(dev), zc.to(dev), want_hit=True)
    assert int(hit.sum()) == 0 and bool((span.cpu() == torch.tensor([B.NEAR, B.FAR])).all())
    assert same_bits(z_c, zc.unsqueeze(0) + jit.unsqueeze(1))


def test_ray_depths_write_nothing_beyond_their_rows(gpu_device):
    """N = 65 rays (a part-filled workgroup) into buffers with guard words behind them: the library is called directly."""
    from mc_nerf_amd import _fit
    ops, dev, N, Sc, Sf = _ops(), gpu_device, 65, 65, 130
    o, d, jit, zc, zf = _depths_case("hand", N, Sc, Sf, True)
    on = lambda t: t.to(dev).contiguous()
    bufs = [torch.full((n + 64,), -7.0, device=dev) for n in (N * Sc, N * Sf, N * 2)]
    hit = torch.full((N + 64,), -7, dtype=torch.int32, device=dev)
    _fit.call("mcnerf_fit_ray_depths", on(o), on(d), N, torch.tensor(B.BOX, device=dev), B.NEAR, B.FAR, on(jit), on(zc), Sc, on(zf), Sf, *bufs, hit, ops._stream())
    torch.cuda.synchronize()
    for buf, n in zip(bufs, (N * Sc, N * Sf, N * 2)):
        assert bool((buf[n:] == -7.0).all()) and bool((buf[:n] != -7.0).all())
    assert bool((hit[N:] == -7).all()) and bool(((hit[:N] == 0) | (hit[:N] == 1)).all())


@pytest.mark.parametrize("margin", [0, 2])
def test_the_fitted_box_goes_straight_into_ray_depths(gpu_device, margin):
    """voxel_box -> ray_depths on one stream, the box never copied: the rows are those of the restatement's box given as a tuple."""
    ops, dev, G = _ops(), gpu_device, 16
    vox = F.blob(G, (5, 6, 7), (9, 9, 10))
    grid = _grid(dev, vox)
    d, o = B.model_rays(257)
    g = torch.Generator().manual_seed(1)
    jit = torch.rand(257, generator=g) * 7.0 / 64
    zc, zf = torch.linspace(B.NEAR, B.FAR, 64).to(dev), torch.linspace(B.NEAR, B.FAR, 128).to(dev)
    cells, box = ops.voxel_box(grid, 0.0, margin, CUBE)
    got = ops.ray_depths(o.to(dev), d.to(dev), box, B.NEAR, B.FAR, jit.to(dev), zc, zf, want_hit=True)
    r_cells, r_box = F.voxel_box_ref(vox, grid.bmin, grid.h, 0.0, margin, CUBE)
    want = ops.ray_depths(o.to(dev), d.to(dev), tuple(r_box.tolist()), B.NEAR, B.FAR, jit.to(dev), zc, zf, want_hit=True)
    assert torch.equal(cells.cpu(), r_cells) and same_bits(box, r_box) and int(r_cells[6]) == 1
    for a, b in zip(got, want):
        assert same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)
    assert 0 < int(got[3].sum()) < 257                                          # some rays hit the fitted box, some miss it
    # a refit in place, of an emptied grid: the same tensor now holds the outer box
    grid.vox.fill_(-1.0)
    ops.voxel_box(grid, 0.0, margin, CUBE, cells, box)
    assert box.tolist() == list(CUBE) and cells.tolist() == [G, G, G, -1, -1, -1, 0, 0]
