"""Error-guided pixel sampling (`pixel_sampler` = "error") without a GPU: the sys_param keys at model construction, the
ops' and the model's refusal of host tensors, the C entry points' refusals ahead of any device work, and self-checks of the torch
restatement (tests/errmap_ref.py) that the GPU tests compare against."""
import ctypes

import pytest
import torch

import errmap_ref as R
from mc_nerf_amd import synthetic as S

SHAPES = [(37, 53, 8), (100, 100, 1), (20, 30, 64), (800, 800, 16)]


def _sys_param(**kw):
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    sp.update(kw)
    return sp


def _model(**kw):
    from mc_nerf_amd.model import MC_Model
    sp = _sys_param(**kw)
    return MC_Model(sp), sp


# ------------------------------------------------------------------------------------------------------------------ the keys
@pytest.mark.parametrize("bad", ["bogus", "Error", "", None, 1, True])
def test_bad_pixel_sampler_is_refused(bad):
    with pytest.raises(ValueError, match="pixel_sampler"):
        _model(pixel_sampler=bad)


@pytest.mark.parametrize("bad", [0, 257, -1, 16.0, "16", None, True])
def test_bad_error_tile_is_refused(bad):
    with pytest.raises(ValueError, match="error_tile"):
        _model(pixel_sampler="error", error_tile=bad)


@pytest.mark.parametrize("bad", [0, 0.0, -0.5, 1.5, float("nan"), float("inf"), "0.5", None, True])
def test_bad_error_beta_is_refused(bad):
    with pytest.raises(ValueError, match="error_beta"):
        _model(pixel_sampler="error", error_beta=bad)


@pytest.mark.parametrize("bad", [-0.1, 1.1, float("nan"), float("inf"), "0.5", None, True])
def test_bad_error_uniform_frac_is_refused(bad):
    with pytest.raises(ValueError, match="error_uniform_frac"):
        _model(pixel_sampler="error", error_uniform_frac=bad)


def test_an_image_above_2_to_the_26_pixels_is_refused_in_error_mode_only():
    with pytest.raises(ValueError, match="data_img_h"):
        _model(pixel_sampler="error", data_img_h=8193, data_img_w=8192)
    from mc_nerf_amd.model import MC_Model
    assert MC_Model._error_settings(_sys_param(data_img_h=8192, data_img_w=8192)) == (16, 0.5, 0.5)


@pytest.mark.parametrize("kw", [{}, {"pixel_sampler": "uniform"}])
def test_keys_are_not_validated_in_uniform_mode_and_nothing_is_allocated(kw):
    from mc_nerf_amd._lib import McnerfError
    m, _ = _model(error_tile=0, error_beta=-1.0, error_uniform_frac="x", **kw)
    assert m.pixel_sampler == "uniform" and m._error_map is None and not hasattr(m, "error_tile")
    assert len(m.state_dict()) == 46
    for call in (m.error_map, m.reset_error_map, m.reserve_error_map):
        with pytest.raises(McnerfError, match="pixel_sampler"):
            call()


def test_error_mode_reads_its_keys_and_adds_nothing_to_the_state_dict():
    base, _ = _model()
    m, _ = _model(pixel_sampler="error")
    assert (m.error_tile, m.error_beta, m.error_uniform_frac) == (16, 0.5, 0.5) and m.draw_error_uniforms(7) is None
    m2, _ = _model(pixel_sampler="error", error_tile=256, error_beta=1, error_uniform_frac=0, color_calib="affine")
    assert (m2.error_tile, m2.error_beta, m2.error_uniform_frac) == (256, 1.0, 0.0)
    assert list(m.state_dict()) == list(base.state_dict()) and len(m2.state_dict()) == 47
    assert m._error_map is None and not any("err" in n for n, _ in list(m.named_buffers()) + list(m.named_parameters()))
    em = m.reserve_error_map()
    assert m.reserve_error_map() is em and em.err.shape == (m.train_numb, 1, 1) and float(em.err.min()) == 1.0
    assert list(m.state_dict()) == list(base.state_dict())
    assert m.error_map().shape == (m.train_numb, 1, 1) and m.error_map(2).shape == (1, 1)
    with pytest.raises(ValueError, match="cam"):
        m.error_map(m.train_numb)


# ------------------------------------------------------------------------------------------------------------------ no fallback
def test_ops_refuse_cpu_tensors():
    from mc_nerf_amd import ops
    from mc_nerf_amd._lib import McnerfError
    em = ops.ErrorMap(3, 20, 30, 8, "cpu")
    assert em.err.shape == em.scratch.shape == (3, 3, 4) and em.cdf.shape == (64, 12) and em.cdf.dtype == torch.int64
    assert float(em.err.min()) == 1.0 and int(em.scratch.abs().max()) == 0
    with pytest.raises(McnerfError):
        ops.errmap_sample(em, [1], [0, 5], 0.5)
    with pytest.raises(McnerfError):
        ops.errmap_sample(em, [1], [0, 5], 0.5, torch.rand(5, 2))
    with pytest.raises(McnerfError):
        ops.errmap_update(em, [1], [0, 5], torch.zeros(5, dtype=torch.int64), torch.rand(5, 3), torch.rand(5, 3), 0.5)
    with pytest.raises(McnerfError):
        ops.errmap_sample(em, [1, 2], [0, 5], 0.5, torch.rand(5, 2))                # K + 1 entries
    for bad in ((0, 20, 30, 8), (3, 20, 30, 0), (3, 8193, 8192, 16)):
        with pytest.raises(McnerfError):
            ops.ErrorMap(*bad, "cpu")


def test_cpu_model_in_error_mode_raises_at_the_step():
    from mc_nerf_amd._lib import McnerfError
    wpts_of = lambda sp: S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    for cams, kw in (([3], {}), ([3, 1], {"cams_per_step": 2})):
        m, sp = _model(pixel_sampler="error", **kw)
        S.init_cameras_near_gt(m)
        wpts, pts = wpts_of(sp)
        with pytest.raises(McnerfError):
            m((torch.rand(len(cams), 8, 8, 3), torch.tensor(cams), wpts, pts, wpts, pts), 20, "GLOBAL_OPTIM_EPOCH", 0.5)


# ------------------------------------------------------------------------------------------------------------------ C refusals
def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


def _sample(l, p, *, C=7, H=20, W=30, tile=8, cams=(0, 1), start=(0, 2, 4), K=2, n=4, frac=0.5, err=True, u=True, cdf=True, pix=True, seg=True):
    q = lambda on: p if on else None
    return l.mcnerf_errmap_sample(q(err), C, H, W, tile, _i32(cams) if seg else None, _i32(start) if seg else None, K, n, frac, q(u), q(cdf),
                                  q(pix), None)


def _update(l, p, *, C=7, H=20, W=30, tile=8, cams=(0, 1), start=(0, 2, 4), K=2, n=4, beta=0.5, omb=0.5, err=True, scratch=True, pix=True,
            rgb=True, gt=True, seg=True):
    q = lambda on: p if on else None
    return l.mcnerf_errmap_update(q(err), q(scratch), C, H, W, tile, _i32(cams) if seg else None, _i32(start) if seg else None, K, n, q(pix),
                                  q(rgb), q(gt), beta, omb, None)


BAD = {                                         # refused by both entry points (C = 7)
    "K = 0": dict(cams=[0], start=[0, 4], K=0),
    "K = 65": dict(cams=[0] * 65, start=list(range(66)), K=65, n=65),
    "camera id = C": dict(cams=[0, 7]),
    "camera id < 0": dict(cams=[-1, 2]),
    "decreasing start": dict(cams=[0, 1, 2], start=[0, 3, 2, 4], K=3),
    "start[0] != 0": dict(start=[1, 2, 4]),
    "start[K] != n": dict(start=[0, 2, 5]),
    "tile = 0": dict(tile=0),
    "H W > 2^26": dict(H=8193, W=8192),
    "no table": dict(seg=False),
    "no map": dict(err=False),
    "no pixels": dict(pix=False),
}
BAD_SAMPLE = {"frac < 0": dict(frac=-0.01), "frac > 1": dict(frac=1.01), "frac NaN": dict(frac=float("nan")), "no u": dict(u=False),
              "no cdf": dict(cdf=False)}
BAD_UPDATE = {"beta > 1": dict(beta=1.5), "beta NaN": dict(beta=float("nan")), "1 - beta < 0": dict(omb=-0.5), "no scratch": dict(scratch=False),
              "no rgb": dict(rgb=False), "no gt": dict(gt=False)}


@pytest.mark.parametrize("case", sorted(BAD) + sorted(BAD_SAMPLE))
def test_sample_entry_point_refuses_without_a_gpu(case):
    """The refusals sit ahead of any HIP call: non-zero on a machine without a GPU.  The device pointers are never read: a host
    buffer stands in for them."""
    from mc_nerf_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    rc = _sample(l, ctypes.addressof(buf), **{**BAD, **BAD_SAMPLE}[case])
    assert rc != 0 and b"mcnerf_errmap_sample: invalid argument" in l.mcnerf_last_error(), case
    assert buf.raw == bytes(4096)


@pytest.mark.parametrize("case", sorted(BAD) + sorted(BAD_UPDATE))
def test_update_entry_point_refuses_without_a_gpu(case):
    from mc_nerf_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    rc = _update(l, ctypes.addressof(buf), **{**BAD, **BAD_UPDATE}[case])
    assert rc != 0 and b"mcnerf_errmap_update: invalid argument" in l.mcnerf_last_error(), case
    assert buf.raw == bytes(4096)


def test_new_files_stay_outside_the_digested_kernel_sources():
    import os
    import bench
    from mc_nerf_amd import build
    assert "errmap.hip" in build.SOURCES and {"mcnerf_errmap.h", "mcnerf_maxkey.h"} <= set(build.HEADERS)
    new = ("errmap.hip", "mcnerf_errmap.h", "mcnerf_maxkey.h")
    assert not set(new) & set(bench.MLP_KERNEL_SOURCES)
    for f in bench.MLP_KERNEL_SOURCES + ("mcnerf_multicam.h", "mcnerf_voxel.h"):
        text = open(os.path.join(build.CSRC, f)).read()
        assert "mcnerf_errmap.h" not in text and "mcnerf_maxkey.h" not in text, f
    # the key functions are stated once
    assert sum("unsigned vox_key(" in open(os.path.join(build.CSRC, f)).read() for f in os.listdir(build.CSRC)) == 1


# ------------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("H, W, tile", SHAPES)
def test_reference_tile_areas_sum_to_the_image(H, W, tile):
    Th, Tw, th, tw = R.tiles(H, W, tile)
    assert (Th, Tw) == (-(-H // tile), -(-W // tile)) and int((th * tw).sum()) == H * W
    assert int(th.min()) >= 1 and int(tw.min()) >= 1 and int(th.max()) <= tile and int(tw.max()) <= tile
    q = R.weights(torch.ones(Th, Tw), H, W, tile)
    assert int(q.sum()) == (1 << 24) * H * W


def test_reference_weights_clamp_and_never_vanish():
    E = torch.tensor([[float("nan"), float("inf"), -3.0, 0.0], [1e-30, 1.0, 4.5, float("-inf")]])
    q = R.weights(E, 2, 4, 1)
    assert q.tolist() == [1, 4 << 24, 1, 1, 1, 1 << 24, 4 << 24, 1]
    assert R.unit(torch.tensor([0.0, 1.0, -0.5, 2.0, float("nan"), 0.25])).tolist() == [0.0, R.ONE_BELOW, 0.0, R.ONE_BELOW, 0.0, 0.25]
    assert R.ONE_BELOW < 1.0 and R.ONE_BELOW == 1.0 - 2.0 ** -24


@pytest.mark.parametrize("H, W, tile", SHAPES)
def test_reference_draws_stay_inside_the_image_and_concentrate_on_a_hot_tile(H, W, tile):
    g = torch.Generator().manual_seed(H + tile)
    Th, Tw, _, _ = R.tiles(H, W, tile)
    n = 100_000
    u = torch.rand(n, 2, generator=g)
    u[:5] = torch.tensor([[0.0, 0.0], [R.ONE_BELOW, R.ONE_BELOW], [1.0, 1.0], [-0.5, 2.0], [float("nan"), float("nan")]])
    E = torch.rand(2, Th, Tw, generator=g) * 5 - 0.5
    E.view(-1)[:: 7] = float("nan")
    E.view(-1)[3:: 11] = float("inf")
    E.view(-1)[5:: 13] = float("-inf")
    pix = R.sample(E, H, W, tile, [1, 0], [0, n // 2, n], 0.3, u)
    assert int(pix.min()) >= 0 and int(pix.max()) < H * W
    # One hot tile at E = 1 among tiles at E = 0: a cold tile keeps the weight 1 * area, so the cold tiles together hold
    # (H W - area_hot) / (2^24 area_hot + H W - area_hot) < 0.01 of the mass at every shape here, on either side of the hot tile's
    # interval of the CDF: every draw with u0 in [0.01, 0.99] lands in the hot tile (u0 = 0 is the first pixel of tile 0 by construction)
    hot = (Th * Tw) // 2
    E = torch.zeros(1, Th, Tw)
    E.view(-1)[hot] = 1.0
    q = R.weights(E[0], H, W, tile)
    assert float(q.sum() - q[hot]) / float(q.sum()) < 0.01
    mid = torch.stack([0.01 + 0.98 * u[:, 0].clamp(0, 1).nan_to_num(0.5), u[:, 1]], 1)
    pix = R.sample(E, H, W, tile, [0], [0, n], 0.0, mid)
    assert bool((R.tile_of(pix, W, tile, Tw) == hot).all())
    assert int(R.sample(E, H, W, tile, [0], [0, n], 0.0, u)[0]) == 0
    # the uniform head of a segment ignores the map
    pix = R.sample(E, H, W, tile, [0], [0, n], 1.0, u)
    assert int(pix.min()) >= 0 and int(pix.max()) < H * W and (Th * Tw == 1 or not bool((R.tile_of(pix, W, tile, Tw) == hot).all()))


def test_reference_update_on_a_case_worked_by_hand():
    """4 x 4 image, tile 2, two cameras; camera 1 in two segments.  Rays: pixel 0 (tile 0) errors 0.25 / 3 and 1 / 3 -> max 1/3; pixel 15
    (tile 3) error 3 * fp32(1/3) = 1 in fp32; a NaN row, pix = -1 and pix = 16 are skipped.  beta = 0.25: E <- 0.75 E + 0.25 m."""
    err = torch.full((2, 2, 2), 2.0)
    pix = torch.tensor([0, 15, 1, 5, -1, 16])
    rgb = torch.tensor([[0.5, 0, 0], [1.0, 1.0, 1.0], [1.0, 0, 0], [float("nan"), 0, 0], [1.0, 1, 1], [1.0, 1, 1]])
    gt = torch.tensor([[0.0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
    out = R.update(err, 4, 4, 2, [1, 0, 1], [0, 2, 2, 6], pix, rgb, gt, 0.25)
    third = float(torch.tensor(1.0) * R.THIRD)
    want0 = float(torch.tensor(0.75) * 2.0 + torch.tensor(0.25) * torch.tensor(third))
    assert torch.equal(out[0], err[0]) and float(out[1, 0, 0]) == want0 and float(out[1, 1, 1]) == 1.75
    assert float(out[1, 0, 1]) == 2.0 and float(out[1, 1, 0]) == 2.0 and float(err.min()) == 2.0
