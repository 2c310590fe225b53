"""The multi-camera train step (`cams_per_step`) without a GPU: the two entry points in the header, the ctypes table and the built
library; `ops.ray_segments`; the sys_param key at model construction; `distributed.group_cameras`; the C entry points' refusal of a
bad segment table ahead of any device work; the ops' refusal of CPU tensors; the fp64 restatement (tests/multicam_ref.py) on a
camera that can be checked by hand."""
import ctypes
import os
import re

import pytest
import torch

import multicam_ref as R
from mc_nerf_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcnerf_ray_batch_fwd", "mcnerf_ray_batch_bwd"]


def _model(**kw):
    from mc_nerf_amd.model import MC_Model
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    sp.update(kw)
    return MC_Model(sp), sp


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_declares_the_ray_batch_entry_points_and_keeps_its_version():
    from mc_nerf_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "mcnerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "rays.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "rays.hip"))
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in SYMBOLS:
        assert f"int {name}(" in code and name in _lib.SIGNATURES and hasattr(lib, name), name
        n_args = code.split(f"int {name}(")[1].split(")")[0].count(",") + 1
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    assert _lib.ABI_VERSION == 7 and "#define MCNERF_ABI_VERSION 7" in hdr and _lib.lib().mcnerf_abi_version() == 7


# ------------------------------------------------------------------------------------------------------------------ segments
def test_ray_segments():
    from mc_nerf_amd import ops
    assert ops.ray_segments(301, 3) == [0, 101, 201, 301]
    assert ops.ray_segments(3, 3) == [0, 1, 2, 3]
    s = ops.ray_segments(7000, 8)
    sizes = [b - a for a, b in zip(s, s[1:])]
    assert len(s) == 9 and s[0] == 0 and sum(sizes) == 7000 and max(sizes) - min(sizes) <= 1
    assert sizes == sorted(sizes, reverse=True)             # the longer segments come first: n_k = q + (k < r)
    assert ops.ray_segments(5, 1) == [0, 5]
    with pytest.raises(ValueError):
        ops.ray_segments(5, 0)


@pytest.mark.parametrize("batch, K", [(301, 3), (3, 3), (7000, 8), (64, 64), (130, 64), (5, 1)])
def test_ray_segment_index_agrees_with_the_table(batch, K):
    from mc_nerf_amd import ops
    s = ops.ray_segments(batch, K)
    want = torch.cat([torch.full((b - a,), k, dtype=torch.int64) for k, (a, b) in enumerate(zip(s, s[1:]))])
    assert torch.equal(ops.ray_segment_index(batch, K, "cpu"), want)


# ------------------------------------------------------------------------------------------------------------------ the key
@pytest.mark.parametrize("bad", [True, 0, 65, 2.0, 17, -1, "2", None])
def test_bad_cams_per_step_is_refused(bad):
    with pytest.raises(ValueError, match="cams_per_step"):          # (17 = batch + 1)
        _model(cams_per_step=bad)


def test_cams_per_step_defaults_to_one_camera():
    m, _ = _model()
    assert m.cams_per_step == 1 and m.sample_pixels_multi(64, [0, 16]) is None
    m, _ = _model(cams_per_step=16)
    assert m.cams_per_step == 16
    assert _model(batch=64, cams_per_step=64)[0].cams_per_step == 64


def _cpu_data(sp, cams, H=8, W=8):
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    return (torch.rand(len(cams), H, W, 3), torch.tensor(cams), wpts, pts, wpts, pts)


def test_cpu_model_has_no_multicamera_fallback():
    from mc_nerf_amd._lib import McnerfError
    m, sp = _model(cams_per_step=2)
    S.init_cameras_near_gt(m)
    with pytest.raises(McnerfError):
        m(_cpu_data(sp, [3, 1]), 20, "GLOBAL_OPTIM_EPOCH", 0.5)
    with pytest.raises(ValueError, match="camera ids"):
        m(_cpu_data(sp, [3, 1, 2]), 20, "GLOBAL_OPTIM_EPOCH", 0.5)
    with pytest.raises(ValueError, match="camera ids"):
        m(_cpu_data(sp, [3]), 20, "FINE_TUNE_EPOCH", 0.5)
    # the camera-only stage has no rays: unchanged, one id or K (its validation rays come from the HIP ray generator: stubbed)
    m.get_rays = lambda pose, img_id, intr_inv: (torch.zeros(64, 3), torch.zeros(64, 3))
    loss_dict, *_ = m(_cpu_data(sp, [3]), 1, "CAM_PARAM_EPOCH", 0.0)
    assert set(loss_dict) == {"intr", "extr"}


def test_ops_refuse_cpu_tensors():
    from mc_nerf_amd import ops
    from mc_nerf_amd._lib import McnerfError
    pose, kinv = torch.zeros(4, 3, 4), torch.zeros(4, 3, 3)
    with pytest.raises(McnerfError):
        ops.ray_batch_fwd(pose, kinv, [1, 2], [0, 3, 6], 4, 4)
    with pytest.raises(McnerfError):
        ops.ray_batch_bwd(pose, kinv, [1, 2], [0, 3, 6], 4, torch.zeros(6, dtype=torch.int64), torch.zeros(6, 3), torch.zeros(6, 3))
    with pytest.raises(McnerfError):
        ops.ray_batch_fwd(pose, kinv, [1, 2], [0, 3], 4, 4)          # seg_start needs K + 1 entries


# ------------------------------------------------------------------------------------------------------------------ the table
def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


BAD_TABLES = {                                  # (seg_cam, seg_start, K, n) with C = 7, H * W = 16
    "K = 0": ([0], [0, 4], 0, 4),
    "K = 65": ([0] * 65, list(range(66)), 65, 65),
    "camera id = C": ([0, 7], [0, 2, 4], 2, 4),
    "camera id < 0": ([-1, 2], [0, 2, 4], 2, 4),
    "decreasing start": ([0, 1, 2], [0, 3, 2, 4], 3, 4),
    "start[0] != 0": ([0, 1], [1, 2, 4], 2, 4),
    "start[K] != n": ([0, 1], [0, 2, 5], 2, 4),
    "n_k > H W": ([0, 1], [0, 17, 20], 2, 20),
}


@pytest.mark.parametrize("case", sorted(BAD_TABLES))
def test_entry_points_refuse_a_bad_segment_table_without_a_gpu(case):
    """The refusals sit ahead of any HIP call (as mcnerf_param_count's): non-zero on a machine without a GPU.  The device pointers
    are never read: a host buffer stands in for them."""
    from mc_nerf_amd import _lib
    l = _lib.lib()
    cams, start, K, n = BAD_TABLES[case]
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    rc = l.mcnerf_ray_batch_fwd(p, p, 7, _i32(cams), _i32(start), K, n, 4, 4, None, p, None, 0, p, p, p, None, None)
    assert rc != 0 and b"mcnerf_ray_batch_fwd: invalid argument" in l.mcnerf_last_error(), case
    if case != "n_k > H W":                     # (the backward draws nothing: any segment length up to n is legal there)
        rc = l.mcnerf_ray_batch_bwd(p, p, 7, _i32(cams), _i32(start), K, n, 4, p, p, p, p, p, None)
        assert rc != 0 and b"mcnerf_ray_batch_bwd: invalid argument" in l.mcnerf_last_error(), case


def test_entry_point_refuses_bad_channels_without_a_gpu():
    from mc_nerf_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    for ch in (0, 1, 2, 5):
        assert l.mcnerf_ray_batch_fwd(p, p, 7, _i32([0, 1]), _i32([0, 2, 4]), 2, 4, 4, 4, None, p, p, ch, p, p, p, p, None) != 0
        assert b"invalid argument" in l.mcnerf_last_error()


# ------------------------------------------------------------------------------------------------------------------ grouping
def test_group_cameras():
    from mc_nerf_amd.distributed import group_cameras, shard_cameras
    shards = [shard_cameras(10, epoch=3, rank=r, world=3) for r in range(3)]
    groups = [group_cameras(s, 4) for s in shards]
    assert len({len(g) for g in groups}) == 1                        # every rank takes the same number of steps
    for s, g in zip(shards, groups):
        assert all(len(t) == 4 for t in g)
        assert set(s) == {c for t in g for c in t}                   # every id of the shard appears
        flat = [c for t in g for c in t]
        assert flat == [s[i % len(s)] for i in range(len(flat))]     # ... in order, the padding wraps round to the start
    assert group_cameras([7, 8, 9], 2) == [(7, 8), (9, 7)]
    assert group_cameras([7, 8], 5) == [(7, 8, 7, 8, 7)]
    assert group_cameras([1, 2, 3, 4], 2) == [(1, 2), (3, 4)] and group_cameras([1, 2], 1) == [(1,), (2,)]
    with pytest.raises(ValueError):
        group_cameras([1, 2], 0)


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_fp64_reference_on_a_camera_checked_by_hand():
    """Identity rotation, t = (1, 2, 3), Kinv = diag(1/2, 1/4, 1) with principal point (-1, -1): pixel (u, v) = (3, 1) of a
    W = 5 image lifts to cam = ((3.5 / 2) - 1, (1.5 / 4) - 1, 1); o = -t; and the second segment's camera is looked up by id."""
    pose = torch.zeros(3, 3, 4)
    pose[:, :, :3] = torch.eye(3)
    pose[2, :, 3] = torch.tensor([1.0, 2.0, 3.0])
    kinv = torch.zeros(3, 3, 3)
    kinv[:] = torch.tensor([[0.5, 0.0, -1.0], [0.0, 0.25, -1.0], [0.0, 0.0, 1.0]])
    pix = torch.tensor([8, 8])
    d, o = R.rays(pose, kinv, [0, 2], [0, 1, 2], pix, 5)
    q = torch.tensor([0.75, -0.625, 1.0], dtype=torch.float64)
    assert torch.allclose(d[0], q / q.norm()) and torch.allclose(d[1], d[0])
    assert torch.equal(o[0], torch.zeros(3, dtype=torch.float64)) and torch.equal(o[1], -torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64))
    dp, dk = R.backward(pose, kinv, [0, 2], [0, 1, 2], pix, 5, torch.randn(2, 3), torch.ones(2, 3))
    assert float(dp[1].abs().max()) == 0.0 and float(dk[1].abs().max()) == 0.0          # camera 1 is not in the table
    assert torch.equal(dp[2, :, 3], -torch.ones(3, dtype=torch.float64))                # d o / d t = -R
    u8 = torch.tensor([[[255, 0, 51, 51]]], dtype=torch.uint8)
    assert torch.allclose(R.gt_from_u8(u8, 0, torch.tensor([0])), torch.tensor([[1.0, 0.8, 0.84]]))
