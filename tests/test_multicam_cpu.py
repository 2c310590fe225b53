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
        assert f"int {name}(" in code and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 7                             # (new symbols only; tests/test_abi_cpu.py checks header, table and library)


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


# ------------------------------------------------------------------------------------------------------------------ one definition
def _csrc():
    from mc_nerf_amd import build
    return {f: open(os.path.join(build.CSRC, f)).read() for f in sorted(os.listdir(build.CSRC))}


@pytest.mark.parametrize("what, text", [
    ("the lift through the inverse intrinsics", "__fmul_rn(u, K[r * 3])"),
    ("the pose-inverse row of mcn_ray_of_cam", "__fmul_rn(P[0 * 4 + c], P[3])"),
    ("the rotation of mcn_ray_of_cam", "__fmul_rn(cam[0], P[0 * 4 + c])"),
    ("the segment scan", "for (int s = 1; s < t.K; ++s)"),
    ("the longest-segment loop", "for (int k = 0; k < t.K; ++k) longest ="),
    ("the dKinv accumulation", "acc[9 + j * 3 + k] +="),
])
def test_ray_preamble_expressions_are_written_once(what, text):
    """The pinhole and the lens path share one definition: each of these occurs in exactly one file of csrc/, once."""
    hits = {f: s.count(text) for f, s in _csrc().items() if text in s}
    assert len(hits) == 1 and sum(hits.values()) == 1, (what, hits)


def test_compaction_maxblend_and_radam_element_are_written_once():
    """The two ordered lists share one count body and one write body (mcnerf_compact.h), the voxel grid and the error map one
    max / blend pair (mcnerf_maxkey.h), the dense and the row-lazy RAdam one element update (mcnerf_optim_rows.h)."""
    src = _csrc()
    for text, owner in (("atomicExch(", "mcnerf_maxkey.h"), ("sqrtf(vi)", "mcnerf_optim_rows.h")):
        assert [f for f, s in src.items() if text in s] == [owner], text
    for body in ("mcn_compact_count", "mcn_compact_write"):
        assert [f for f, s in src.items() if f"void {body}(" in s] == ["mcnerf_compact.h"], body
        assert sorted(f for f, s in src.items() if f"{body}<" in s) == ["select.hip", "voxel.hip"], body
    for f, names in (("select.hip", ("select_count_kernel", "select_write_kernel")), ("voxel.hip", ("voxel_count_kernel", "voxel_write_kernel", "voxel_max_kernel", "voxel_blend_kernel")),
                     ("errmap.hip", ("errmap_max_kernel", "errmap_blend_kernel"))):
        for name in names:
            m = re.search(r"__global__ __launch_bounds__\(256\) void " + name + r"\(([^)]*)\) \{\n(.*?)\n\}\n", src[f], flags=re.S)
            assert m and len(m.group(2).split("\n")) == 1 and "mcn_c" in m.group(2), (f, name)
    for f in ("optim.hip", "optim_rows.hip"):
        assert src[f].count("mcn_radam_element(") == 1, f


def test_ray_batch_entry_points_stay_in_their_files_as_thin_kernels():
    src = _csrc()
    for f, names in (("rays.hip", ("ray_batch_fwd_kernel", "ray_batch_bwd_kernel")), ("lens.hip", ("lens_ray_batch_fwd_kernel", "lens_ray_batch_bwd_kernel"))):
        for name in names:
            m = re.search(r"__global__ __launch_bounds__\(256\) void " + name + r"\(([^)]*)\) \{\n(.*?)\n\}\n", src[f], flags=re.S)
            assert m and len(m.group(2).split("\n")) <= 3 and "_body<" in m.group(2), (f, name)
            assert sum(("void " + name + "(") in s for s in src.values()) == 1, name
    assert "err_segment" not in src["errmap.hip"] and "mcn_segment_of_ray(" in src["errmap.hip"] and "mcn_segment_of_ray(" in src["mcnerf_rays.h"]


def test_ops_reach_each_ray_batch_symbol_from_one_function_body():
    import ast
    import inspect
    from mc_nerf_amd import ops
    tree = ast.parse(inspect.getsource(ops))
    text = inspect.getsource(ops)
    owners, calls_with_symbol = {}, []
    for fn in [n for n in tree.body if isinstance(n, ast.FunctionDef)]:
        for node in ast.walk(fn):
            if isinstance(node, ast.Constant) and isinstance(node.value, str) and re.fullmatch(r"mcnerf_(lens_)?ray_batch_(fwd|bwd)", node.value):
                owners.setdefault(node.value, []).append(fn.name)
            if isinstance(node, ast.Call) and ast.unparse(node.func) == "_lib.call" and ast.unparse(node.args[0]) == "symbol":
                calls_with_symbol.append(fn.name)
    assert owners == {"mcnerf_ray_batch_fwd": ["ray_batch_fwd"], "mcnerf_ray_batch_bwd": ["ray_batch_bwd"],
                      "mcnerf_lens_ray_batch_fwd": ["lens_ray_batch_fwd"], "mcnerf_lens_ray_batch_bwd": ["lens_ray_batch_bwd"]}
    assert sorted(calls_with_symbol) == ["_ray_batch_bwd", "_ray_batch_fwd"]            # the two private ops are the only callers
    assert text.count("_ray_batch_fwd(\"mcnerf_") == 2 and text.count("_ray_batch_bwd(\"mcnerf_") == 2


# ------------------------------------------------------------------------------------------------------------------ one step
STEP_CONFIGS = [(1, "pinhole", "uniform", 16), (1, "radial", "uniform", 16), (1, "radial", "uniform", 100), (1, "pinhole", "error", 16),
                (1, "radial", "error", 16), (2, "pinhole", "uniform", 16), (2, "radial", "uniform", 16), (2, "pinhole", "error", 16),
                (2, "pinhole", "hook", 16), (2, "radial", "hook+error", 16)]


@pytest.mark.parametrize("K, lens, sampler, batch", STEP_CONFIGS)
@pytest.mark.parametrize("stage", ["GLOBAL_OPTIM_EPOCH", "FINE_TUNE_EPOCH"])
def test_nerf_stage_step_routes_every_configuration(monkeypatch, K, lens, sampler, batch, stage):
    """The one NeRF-stage step on a CPU model with the HIP ops stubbed: which ray op each configuration reaches and with what
    arguments, and what the step leaves behind (8 x 8 images: batch = 100 draws all 64 pixels)."""
    import mc_nerf_amd.model.mc_nerf as M
    error = "error" in sampler
    m, sp = _model(batch=batch, cams_per_step=K, lens_model=lens, color_calib="affine", **({"pixel_sampler": "error"} if error else {}))
    S.init_cameras_near_gt(m)
    cams = [3, 1][:K]
    calls = []

    class Raygen:
        @staticmethod
        def apply(pose, kinv, pix, W):
            calls.append(("raygen", pose, kinv, pix, W))
            return torch.zeros(pix.shape[0], 3), torch.ones(pix.shape[0], 3)

    class RayBatch:
        @staticmethod
        def apply(pose, kinv, seg_cam, seg_start, H, W, images=None, pix=None, seed=None, lens_w=None):
            calls.append(("ray_batch", pose, kinv, lens_w, seg_cam, seg_start, H, W, images, pix))
            out = torch.arange(seg_start[-1]) % (H * W) if pix is None else pix.clone()
            return out, torch.zeros(seg_start[-1], 3), torch.ones(seg_start[-1], 3), None
    monkeypatch.setattr(M, "RaygenFn", Raygen)
    monkeypatch.setattr(M, "RayBatchFn", RayBatch)
    rgb_c, rgb_f = torch.rand(min(batch, 64), 3), torch.rand(min(batch, 64), 3)
    m.nerf.forward = lambda d, o, epoch, ratio: (calls.append(("nerf", d, o, ratio)) or (rgb_c, rgb_f))
    m.get_rays = lambda pose, img_id, intr_inv: (torch.zeros(64, 3), torch.zeros(64, 3))
    drawn = torch.randint(0, 64, (batch,))
    m._draw_error_pixels = lambda c, s: (calls.append(("error_draw", c, s)) or drawn)
    m._update_error_map = lambda *a: calls.append(("error_update",) + a)
    hooked = torch.randint(0, 64, (batch,))
    if "hook" in sampler:
        m.sample_pixels_multi = lambda npix, seg: hooked
    data = _cpu_data(sp, cams)
    joint = stage == "GLOBAL_OPTIM_EPOCH"
    loss_dict, *_ = m(data, 20, stage, 0.5)

    n = min(batch, 64)
    seg = [0, n] if K == 1 else [0, batch // 2, batch]
    names = [c[0] for c in calls]
    ray = "raygen" if (K, lens) == (1, "pinhole") else "ray_batch"
    draws = ["error_draw"] if error and sampler != "hook+error" else []          # (an injected draw wins over the error draw)
    assert names == draws + [ray, "nerf"] + (["error_update"] if error else [])
    op = calls[len(draws)]
    if ray == "raygen":
        pix = op[3]
        assert torch.equal(op[1], m.pose_adj[cams[0]]) and op[4] == 8 and pix.shape == (n,)
    else:
        _, pose, kinv, lens_w, seg_cam, seg_start, H, W, images, pix_in = op
        assert pose is m.pose_adj and kinv.shape == (sp["data_numb"][0], 3, 3) and (H, W) == (8, 8) and images is None
        assert (lens_w is m.weights_lens) if lens == "radial" else lens_w is None
        assert seg_cam == cams and seg_start == seg
        want_in = hooked if "hook" in sampler else drawn if error else None
        if K == 1 and not error:        # the step's own uniform draw, without replacement
            assert pix_in.shape == (n,) and len(set(pix_in.tolist())) == n
        else:
            assert pix_in is want_in
        pix = pix_in if pix_in is not None else torch.arange(batch) % 64
    if error and not draws == []:
        assert calls[0][1:] == (cams, [0, batch] if K == 1 else seg) and torch.equal(pix, drawn)
    nerf = calls[len(draws) + 1]
    assert nerf[1].shape == (n, 3) and nerf[3] == (0.5 if joint else 1)
    want_gt = data[0].reshape(-1, 3)[pix] if K == 1 else data[0].reshape(K, -1, 3)[torch.arange(batch) // (batch // 2), pix]
    assert loss_dict["rgb"][0] is rgb_c and loss_dict["rgb"][1] is rgb_f and torch.equal(loss_dict["rgb"][2], want_gt)
    assert loss_dict["color"][0] is m.weights_color and loss_dict["color"][1:] == [cams, seg] and set(loss_dict) == {"intr", "rgb", "color"}
    assert m.opt_idx == (1 if joint else 2) and m.nerf.emmbedding_xyz.barf_mode is joint
    if K > 1 or error:
        assert m.last_step_segments == (cams, seg) and torch.equal(m.last_step_pix, pix)
    else:
        assert m.last_step_segments is None and m.last_step_pix is None
    if error:
        upd = calls[-1]
        assert upd[1:3] == (cams, seg) and torch.equal(upd[3], pix) and upd[4] is rgb_f and torch.equal(upd[5], want_gt)      # the fine colours


def test_camera_only_stage_takes_the_single_camera_branch_at_any_cams_per_step(monkeypatch):
    import mc_nerf_amd.model.mc_nerf as M
    m, sp = _model(cams_per_step=2, lens_model="radial")
    S.init_cameras_near_gt(m)
    monkeypatch.setattr(M.MC_Model, "_forward_train_nerf", lambda *a, **k: pytest.fail("the NeRF-stage step ran in the camera-only stage"))
    m.get_rays = lambda pose, img_id, intr_inv: (torch.zeros(64, 3), torch.zeros(64, 3))
    loss_dict, *_ = m(_cpu_data(sp, [3, 1]), 1, "CAM_PARAM_EPOCH", 0.0)
    assert set(loss_dict) == {"intr", "extr"} and m.opt_idx == 0 and m.nerf.emmbedding_xyz.barf_mode is False
