"""Error-guided pixel sampling (`pixel_sampler` = "error"; csrc/errmap.hip) on the GPU against the torch restatement of
tests/errmap_ref.py.  Tile weights are integers and every other quantity is one IEEE operation at a time, so the comparisons are
torch.equal throughout.

Shapes (H, W, tile): (37, 53, 8) ragged edge tiles on both axes; (100, 100, 1) T = 10 000 tiles, five chunks of the block scan;
(20, 30, 64) a single tile.  Tables: one segment of 1000 rays; cameras [2, 0, 2] with 334 / 333 / 333 rays; one ray; five rays in
three segments."""
import pytest
import torch

import errmap_ref as R
from mc_nerf_amd import synthetic as S

pytestmark = pytest.mark.gpu
C = 4
SHAPES = {"37x53t8": (37, 53, 8), "100x100t1": (100, 100, 1), "20x30t64": (20, 30, 64)}
TABLES = {"K1n1000": ([1], 1000), "K3n1000": ([2, 0, 2], 1000), "K1n1": ([3], 1), "K3n5": ([2, 0, 2], 5)}
SPECIAL_U = [[0.0, 0.0], [R.ONE_BELOW, R.ONE_BELOW], [1.0, 1.0], [-0.5, 2.0], [float("nan"), float("nan")]]


def _maps(H, W, tile, seed):
    """name -> err [C,Th,Tw] on the host: random; with NaN, +inf, -3, 0 and 1e-30 entries; one-hot (one tile at 1 among zeros)."""
    Th, Tw, _, _ = R.tiles(H, W, tile)
    g = torch.Generator().manual_seed(seed)
    rnd = torch.rand(C, Th, Tw, generator=g) * 2.0
    odd = rnd.clone()
    flat = odd.view(C, -1)
    for i, v in enumerate((float("nan"), float("inf"), -3.0, 0.0, 1e-30)):
        flat[:, i % (Th * Tw)] = v          # (a single tile: the last value stands)
    hot = torch.zeros(C, Th, Tw)
    hot.view(C, -1)[:, (Th * Tw) // 2] = 1.0
    return {"random": rnd, "odd": odd, "one-hot": hot}


def _u(n, seed):
    u = torch.rand(n, 2, generator=torch.Generator().manual_seed(seed))
    u[:min(n, 5)] = torch.tensor(SPECIAL_U)[:n]
    return u


def _emap(dev, H, W, tile, err):
    from mc_nerf_amd import ops
    em = ops.ErrorMap(C, H, W, tile, dev)
    em.err.copy_(err)
    return em


# ------------------------------------------------------------------------------------------------------------------ 1. sample
@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_sample_equals_the_reference(gpu_device, shape, table):
    from mc_nerf_amd import ops
    H, W, tile = SHAPES[shape]
    cams, n = TABLES[table]
    seg = ops.ray_segments(n, len(cams))
    Th, Tw, _, _ = R.tiles(H, W, tile)
    u = _u(n, 11)
    # (one-hot: the cold tiles hold < 1 % of the mass on either side of the hot tile, tests/test_error_sampler_cpu.py: with u0 in
    #  [0.01, 0.99] every error ray lands in the hot tile)
    mid = torch.stack([0.01 + 0.98 * torch.rand(n, generator=torch.Generator().manual_seed(12)), u[:, 1]], 1)
    for name, err in _maps(H, W, tile, 5).items():
        em = _emap(gpu_device, H, W, tile, err)
        before = em.err.clone()
        for frac in (0.0, 0.3, 1.0):
            for draws in (u, mid) if name == "one-hot" else (u,):
                pix = ops.errmap_sample(em, cams, seg, frac, draws.to(gpu_device)).cpu()
                assert pix.dtype == torch.int64 and pix.shape == (n,)
                assert int(pix.min()) >= 0 and int(pix.max()) < H * W, (name, frac)
                assert torch.equal(pix, R.sample(err, H, W, tile, cams, seg, frac, draws)), (name, frac)
                if draws is mid:
                    f32 = R.f32(frac)
                    for a, b in zip(seg, seg[1:]):
                        drawn = pix[a + int(f32 * (b - a)):b]
                        assert bool((R.tile_of(drawn, W, tile, Tw) == (Th * Tw) // 2).all()), (name, frac)
        assert torch.equal(em.err.view(torch.int32), before.view(torch.int32)) and int(em.scratch.abs().max()) == 0
    # the rows of the workspace are the inclusive integer prefix sums of the segments' cameras
    cdf = em.cdf[:len(cams)].cpu()
    for k, cam in enumerate(cams):
        assert torch.equal(cdf[k], torch.cumsum(R.weights(err[cam], H, W, tile), 0))


def test_sample_draws_its_own_uniforms_from_the_device_generator(gpu_device):
    from mc_nerf_amd import ops
    H, W, tile = SHAPES["37x53t8"]
    err = _maps(H, W, tile, 5)["random"]
    em = _emap(gpu_device, H, W, tile, err)
    torch.manual_seed(21)
    a = ops.errmap_sample(em, [2, 0, 2], [0, 334, 667, 1000], 0.3)
    torch.manual_seed(21)
    u = torch.rand(1000, 2, device=gpu_device)
    assert torch.equal(a.cpu(), R.sample(err, H, W, tile, [2, 0, 2], [0, 334, 667, 1000], 0.3, u.cpu()))


# ------------------------------------------------------------------------------------------------------------------ 2. update
@pytest.mark.parametrize("beta", [1.0, 0.25])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_update_equals_the_reference_and_does_not_depend_on_the_order(gpu_device, shape, beta):
    from mc_nerf_amd import ops
    H, W, tile = SHAPES[shape]
    cams, n = [2, 0, 2], 1000                   # camera 2 in two segments; cameras 1 and 3 absent
    seg = ops.ray_segments(n, 3)
    g = torch.Generator().manual_seed(31)
    err = torch.rand(C, *R.tiles(H, W, tile)[:2], generator=g) * 2.0
    err[1].view(-1)[0] = float("nan")           # an absent camera's rows keep their bits, whatever they are
    err[3].view(-1)[-1] = float("-inf")
    pix = torch.randint(0, H * W, (n,), generator=g)
    pix[:40] = pix[0]                           # several rays in one tile (and all 1000 in it at the single-tile shape)
    pix[500], pix[501] = -1, H * W
    rgb, gt = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    rgb[7, 1], rgb[8, 0], gt[9, 2] = float("nan"), float("inf"), float("-inf")
    want = R.update(err, H, W, tile, cams, seg, pix, rgb, gt, beta)
    em = _emap(gpu_device, H, W, tile, err)
    ops.errmap_update(em, cams, seg, pix.to(gpu_device), rgb.to(gpu_device), gt.to(gpu_device), beta)
    got = em.err.cpu()
    assert torch.equal(got[[0, 2]], want[[0, 2]]) and not torch.equal(got[[0, 2]], err[[0, 2]])
    assert torch.equal(got[[1, 3]].view(torch.int32), err[[1, 3]].view(torch.int32))
    touched = torch.zeros(C, got[0].numel(), dtype=torch.bool)
    Tw = R.tiles(H, W, tile)[1]
    e = R.ray_error(rgb, gt)
    for k, cam in enumerate(cams):
        for i in range(seg[k], seg[k + 1]):
            if 0 <= int(pix[i]) < H * W and bool(torch.isfinite(e[i])):
                touched[cam, int(R.tile_of(pix[i], W, tile, Tw))] = True
    assert torch.equal(got.view(C, -1)[~touched].view(torch.int32), err.view(C, -1)[~touched].view(torch.int32))
    assert int(em.scratch.abs().max()) == 0
    # the same rays in another order within each segment
    perm = torch.cat([a + torch.randperm(b - a, generator=g) for a, b in zip(seg, seg[1:])])
    em2 = _emap(gpu_device, H, W, tile, err)
    ops.errmap_update(em2, cams, seg, pix[perm].to(gpu_device), rgb[perm].to(gpu_device), gt[perm].to(gpu_device), beta)
    assert torch.equal(em2.err.view(torch.int32), em.err.view(torch.int32)) and int(em2.scratch.abs().max()) == 0
    # a second update on the first one's map: the scratch words were left at zero
    ops.errmap_update(em, cams, seg, pix.to(gpu_device), rgb.to(gpu_device), gt.to(gpu_device), beta)
    assert torch.equal(em.err.cpu()[[0, 2]], R.update(want, H, W, tile, cams, seg, pix, rgb, gt, beta)[[0, 2]])


# ------------------------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_leave_the_output_buffers_untouched(gpu_device):
    from mc_nerf_amd import _lib, ops
    from mc_nerf_amd.ops import _seg_arrays, _stream
    H, W, tile, n = 37, 53, 8, 6
    em = _emap(gpu_device, H, W, tile, _maps(H, W, tile, 5)["random"])
    em.cdf.fill_(-7)
    u = torch.rand(n, 2, device=gpu_device)
    pix = torch.full((n,), -5, dtype=torch.int64, device=gpu_device)
    rgb, gt = torch.rand(n, 3, device=gpu_device), torch.rand(n, 3, device=gpu_device)
    err0 = em.err.clone()

    def sample(cams=(0, 1), start=(0, 3, 6), n_=n, geom=(C, H, W, tile), frac=0.5, err=True, u_=True, cdf=True, out=True):
        cs, st, K, _ = _seg_arrays(cams, start)
        q = lambda t, on: t if on else None
        _lib.call("mcnerf_errmap_sample", q(em.err, err), *geom, cs, st, K, n_, frac, q(u, u_), q(em.cdf, cdf),
                  q(pix, out), _stream())

    def update(cams=(0, 1), start=(0, 3, 6), n_=n, geom=(C, H, W, tile), beta=0.5, omb=0.5, err=True, scratch=True, p=True, c=True, g=True):
        cs, st, K, _ = _seg_arrays(cams, start)
        q = lambda t, on: t if on else None
        _lib.call("mcnerf_errmap_update", q(em.err, err), q(em.scratch, scratch), *geom, cs, st, K, n_, q(pix, p),
                  q(rgb, c), q(gt, g), beta, omb, _stream())

    tables = [dict(cams=(), start=(0,), n_=0), dict(cams=(0,) * 65, start=tuple(range(66)), n_=65), dict(cams=(0, C)), dict(cams=(-1, 1)),
              dict(start=(0, 4, 3)), dict(start=(1, 3, 6)), dict(start=(0, 3, 5)), dict(n_=7),
              dict(geom=(C, H, W, 0)), dict(geom=(C, 8193, 8192, 16))]
    for kw in tables + [dict(frac=-0.1), dict(frac=1.5), dict(frac=float("nan")), dict(err=False), dict(u_=False), dict(cdf=False), dict(out=False)]:
        with pytest.raises(_lib.McnerfError, match="mcnerf_errmap_sample"):
            sample(**kw)
    for kw in tables + [dict(beta=1.5), dict(beta=float("nan")), dict(err=False), dict(scratch=False), dict(p=False), dict(c=False), dict(g=False)]:
        with pytest.raises(_lib.McnerfError, match="mcnerf_errmap_update"):
            update(**kw)
    with pytest.raises(_lib.McnerfError):
        ops.errmap_sample(em, [0, 1], [0, 3, 6], 0.5, u[:5])
    with pytest.raises(_lib.McnerfError):
        ops.errmap_update(em, [0, 1], [0, 3, 6], pix, rgb[:5], gt, 0.5)
    assert bool((pix == -5).all()) and bool((em.cdf == -7).all()) and int(em.scratch.abs().max()) == 0
    assert torch.equal(em.err.view(torch.int32), err0.view(torch.int32))
    sample()                                    # ... and the same buffers serve a good call
    assert int(pix.min()) >= 0 and int(pix.max()) < H * W


# ------------------------------------------------------------------------------------------------------------------ 4. the model
STAGE = "GLOBAL_OPTIM_EPOCH"
H_, W_, TILE, BATCH = 32, 48, 8, 256
STEP_CAMS = [5, 0, 5]
FRAC, BETA = 0.3, 0.25


def _step_setup(dev, K, **extra):
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model
    if K > 1:
        extra["cams_per_step"] = K
    sp = S.make_sys_param(dev, samples=32, scale=2, batch=BATCH, H=H_, W=W_, coarse=(4, 32, [2]), fine=(4, 64, [2]), precision="f16x3h", **extra)
    torch.manual_seed(3)
    model = MC_Model(sp).to(dev)
    S.init_cameras_near_gt(model)
    u8 = torch.randint(0, 256, (model.train_numb, H_ * W_, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    data = (DeviceImageSet(u8.to(dev), H_, W_), torch.tensor(STEP_CAMS[:K]), wpts, pts, wpts, pts)
    return sp, model, data


def _seen_colours(model, loss_dict, cams, seg):
    """The fine render as the loss sees it, on the host: per segment (1 + w[c, :3]) * rgb + w[c, 3:] with color_calib = "affine"."""
    rgb = loss_dict["rgb"][1].detach().cpu().clone()
    if model.color_calib == "affine":
        w = model.weights_color.detach().cpu()
        for c, a, b in zip(cams, seg, seg[1:]):
            rgb[a:b] = (1.0 + w[c, :3]) * rgb[a:b] + w[c, 3:]
    return rgb


@pytest.mark.parametrize("calib", ["none", "affine"])
@pytest.mark.parametrize("K", [1, 3])
def test_model_step_draws_from_the_map_and_teaches_it(gpu_device, K, calib):
    from mc_nerf_amd import ops
    extra = {"color_calib": "affine"} if calib == "affine" else {}
    sp, model, data = _step_setup(gpu_device, K, pixel_sampler="error", error_tile=TILE, error_beta=BETA, error_uniform_frac=FRAC, **extra)
    keys = list(model.state_dict())
    plain = list(_step_setup(gpu_device, K)[1].state_dict())             # (4 x 32 / 4 x 64 nets: 38 keys where the full-size nets have 46)
    assert sorted(keys) == sorted(plain + (["weights_color"] if calib == "affine" else []))
    if calib == "affine":
        with torch.no_grad():
            model.weights_color.copy_(0.6 * torch.rand(model.train_numb, 6, generator=torch.Generator().manual_seed(8)) - 0.3)
    called = []
    model.sample_pixels = lambda npix: called.append(npix)          # (not called in error mode)
    em = model.reserve_error_map()
    Th, Tw, _, _ = R.tiles(H_, W_, TILE)
    assert em.err.shape == (model.train_numb, Th, Tw) and float(model.error_map().min()) == 1.0
    em.err.copy_(torch.rand(model.train_numb, Th, Tw, generator=torch.Generator().manual_seed(9)) * 2.0)
    cams, seg = STEP_CAMS[:K], ops.ray_segments(BATCH, K)
    for step in range(2):                       # the second step draws from the map the first one left
        before = model.error_map().cpu()
        u = torch.rand(BATCH, 2, generator=torch.Generator().manual_seed(40 + step))
        model.draw_error_uniforms = lambda n, u=u: u[:n].to(gpu_device)
        torch.manual_seed(7 + step)
        loss_dict, *_ = model(data, 20, STAGE, 0.5)
        assert set(loss_dict) == ({"intr", "rgb", "color"} if calib == "affine" else {"intr", "rgb"})
        assert model.last_step_segments == (cams, seg)
        pix = model.last_step_pix.cpu()
        assert torch.equal(pix, R.sample(before, H_, W_, TILE, cams, seg, FRAC, u)), step
        gt = loss_dict["rgb"][2].detach().cpu()
        assert loss_dict["rgb"][1].shape == (BATCH, 3) and bool(torch.isfinite(loss_dict["rgb"][1]).all())
        want = R.update(before, H_, W_, TILE, cams, seg, pix, _seen_colours(model, loss_dict, cams, seg), gt, BETA)
        after = model.error_map().cpu()
        assert torch.equal(after, want) and not torch.equal(after, before), step
        assert torch.equal(model.error_map(cams[0]).cpu(), want[cams[0]]) and int(em.scratch.abs().max()) == 0
    assert not called and list(model.state_dict()) == keys
    model.reset_error_map()
    assert float(model.error_map().min()) == 1.0 and float(model.error_map().max()) == 1.0


def test_an_injected_multi_camera_draw_still_wins(gpu_device):
    from mc_nerf_amd import ops
    sp, model, data = _step_setup(gpu_device, 3, pixel_sampler="error", error_tile=TILE)
    seg = ops.ray_segments(BATCH, 3)
    mine = torch.randint(0, H_ * W_, (BATCH,), generator=torch.Generator().manual_seed(2)).to(gpu_device)
    model.sample_pixels_multi = lambda npix, seg_start: mine
    model.draw_error_uniforms = lambda n: pytest.fail("an injected draw wins: no uniforms are asked for")
    before = model.error_map().cpu()
    loss_dict, *_ = model(data, 20, STAGE, 0.5)
    assert torch.equal(model.last_step_pix, mine)
    want = R.update(before, H_, W_, TILE, STEP_CAMS, seg, mine.cpu(), loss_dict["rgb"][1].detach().cpu(), loss_dict["rgb"][2].cpu(), 0.5)
    assert torch.equal(model.error_map().cpu(), want)


@pytest.mark.parametrize("K", [1, 3])
def test_without_the_key_the_step_is_todays(gpu_device, K):
    from mc_nerf_amd import ops
    runs = []
    for extra in ({}, {"pixel_sampler": "uniform"}):
        sp, model, data = _step_setup(gpu_device, K, **extra)
        drawn, orig = [], model.sample_pixels
        model.sample_pixels = lambda npix: drawn.append(orig(npix)) or drawn[-1]
        torch.manual_seed(7)
        loss_dict, *_ = model(data, 20, STAGE, 0.5)
        assert model._error_map is None and set(loss_dict) == {"intr", "rgb"}
        if K == 1:
            assert model.last_step_pix is None and model.last_step_segments is None and len(drawn) == 1
            torch.manual_seed(7)
            assert torch.equal(drawn[0], ops.sample_perm(H_ * W_, BATCH, gpu_device))
            pix = drawn[0]
        else:
            assert not drawn
            pix = model.last_step_pix
        runs.append((list(model.state_dict()), pix, *[t.detach() for t in loss_dict["rgb"]]))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) == 38
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(a, b)
