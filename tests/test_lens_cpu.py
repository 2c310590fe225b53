"""The per-camera radial lens model (`lens_model`) without a GPU: the two entry points in the header, the ctypes table
and the built library; the sys_param key at model construction; the refusals of both entry points ahead of any device work; the
fp64 restatement (tests/lens_ref.py) checked against itself, against finite differences and against the formulas the kernel uses; the
eager reprojection op; the camera-only stage of a CPU model; the synthetic data's defaults; the gradient plumbing."""
import ctypes
import os
import re

import pytest
import torch

import lens_ref as R
from mc_nerf_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD = "mcnerf_lens_ray_batch_fwd", "mcnerf_lens_ray_batch_bwd"


def _model(**kw):
    from mc_nerf_amd.model import MC_Model
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    sp.update(kw)
    return MC_Model(sp), sp


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_declares_the_lens_ray_batch_pair_and_keeps_its_version():
    from mc_nerf_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "mcnerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "lens.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "lens.hip"))
    assert "mcnerf_lens.h" in build.HEADERS and os.path.isfile(os.path.join(build.CSRC, "mcnerf_lens.h"))
    lib = ctypes.CDLL(build.build(verbose=False))
    for name, extra in ((FWD, 1), (BWD, 2)):
        assert f"int {name}(" in code and hasattr(lib, name)
        plain = name.replace("lens_", "")                    # the pinhole sibling plus lens (and d_lens)
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[plain][1]) + extra
        names = [p[0] for p in _lib.PARAMS[name][1]]
        assert [n for n in names if n not in ("lens", "d_lens")] == [p[0] for p in _lib.PARAMS[plain][1]] and names[2] == "lens"
    assert _lib.ABI_VERSION == 7                             # (new symbols only; tests/test_abi_cpu.py checks header, table and library)


def test_digested_kernel_sources_do_not_include_the_new_files():
    import bench
    from mc_nerf_amd import build
    assert not {"lens.hip", "mcnerf_lens.h", "mcnerf_rays.h"} & set(bench.MLP_KERNEL_SOURCES)
    for f in bench.MLP_KERNEL_SOURCES:
        text = open(os.path.join(build.CSRC, f)).read()
        assert "mcnerf_lens" not in text and "lens.hip" not in text, f
    # the undistortion is stated once, in its own header
    owner = [f for f in os.listdir(build.CSRC) if "mcn_lens_undistort_radius(float" in open(os.path.join(build.CSRC, f)).read()]
    assert owner == ["mcnerf_lens.h"]


# ------------------------------------------------------------------------------------------------------------------ the key
@pytest.mark.parametrize("bad", ["fisheye", "Radial", "PINHOLE", True, 1, None, "", ["radial"]])
def test_bad_lens_model_is_refused(bad):
    with pytest.raises(ValueError, match="lens_model"):
        _model(lens_model=bad)


@pytest.mark.parametrize("kw", [{}, {"lens_model": "pinhole"}])
def test_default_model_has_the_46_keys_and_no_lens_parameter(kw):
    m, _ = _model(**kw)
    sd = m.state_dict()
    assert m.lens_model == "pinhole" and len(sd) == 46 and not any("weights_lens" in k for k in sd) and not hasattr(m, "weights_lens")
    with pytest.raises(ValueError, match="lens_model"):
        m.lens_coefficients()
    with pytest.raises(ValueError, match="lens_model"):
        m.train_camera_rays(0)


def test_radial_model_adds_one_zero_parameter():
    m, sp = _model(lens_model="radial")
    base, _ = _model()
    C = sp["data_numb"][0]
    sd = m.state_dict()
    assert len(sd) == 47 and set(sd) - set(base.state_dict()) == {"weights_lens"}
    assert m.weights_lens.shape == (C, 2) and m.weights_lens.requires_grad and torch.equal(m.weights_lens.detach(), torch.zeros(C, 2))
    k = m.lens_coefficients()
    assert torch.equal(k, torch.zeros(C, 2)) and not k.requires_grad and k.data_ptr() != m.weights_lens.data_ptr()
    both, _ = _model(lens_model="radial", color_calib="affine")
    assert len(both.state_dict()) == 48
    from mc_nerf_amd.model import NeRF_Model
    for coarse in (True, False):
        assert set(NeRF_Model.rewrite_nerf_ckpt({"model_nerf": sd}, coarse=coarse)) == set(NeRF_Model.rewrite_nerf_ckpt({"model_nerf": base.state_dict()}, coarse=coarse))


# ------------------------------------------------------------------------------------------------------------------ refusals
def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


BAD_TABLES = {                                  # (seg_cam, seg_start, K, n) with C = 7
    "K = 0": ([0], [0, 4], 0, 4),
    "K = 65": ([0] * 65, list(range(66)), 65, 65),
    "camera id = C": ([0, 7], [0, 2, 4], 2, 4),
    "camera id < 0": ([-1, 2], [0, 2, 4], 2, 4),
    "decreasing start": ([0, 1, 2], [0, 3, 2, 4], 3, 4),
    "start[0] != 0": ([0, 1], [1, 2, 4], 2, 4),
    "start[K] != n": ([0, 1], [0, 2, 5], 2, 4),
}
FWD_PTRS = ["pose", "kinv", "lens", "pix_out", "rays_d", "rays_o", "gt"]
BWD_PTRS = ["pose", "kinv", "lens", "pix", "d_rays_d", "d_rays_o", "d_pose", "d_kinv", "d_lens"]


def _fwd(l, p, cams, start, K, n, *, H=4, W=4, channels=4, draw=False, seg=True, missing=()):
    q = lambda name: None if name in missing else p
    return l.mcnerf_lens_ray_batch_fwd(q("pose"), q("kinv"), q("lens"), 7, _i32(cams) if seg else None, _i32(start) if seg else None, K, n, H, W,
                                       None if draw else p, q("seed") if draw else None, p, channels, q("pix_out"), q("rays_d"), q("rays_o"),
                                       q("gt"), None)


def _bwd(l, p, cams, start, K, n, *, W=4, seg=True, missing=()):
    q = lambda name: None if name in missing else p
    return l.mcnerf_lens_ray_batch_bwd(q("pose"), q("kinv"), q("lens"), 7, _i32(cams) if seg else None, _i32(start) if seg else None, K, n, W,
                                       q("pix"), q("d_rays_d"), q("d_rays_o"), q("d_pose"), q("d_kinv"), q("d_lens"), None)


@pytest.mark.parametrize("case", sorted(BAD_TABLES))
def test_entry_points_refuse_a_bad_segment_table_without_a_gpu(case):
    """The refusals sit ahead of any HIP call: non-zero on a machine without a GPU.  The device pointers are never read: a host
    buffer stands in for them."""
    from mc_nerf_amd import _lib
    l = _lib.lib()
    cams, start, K, n = BAD_TABLES[case]
    p = ctypes.addressof(ctypes.create_string_buffer(4096))
    assert _fwd(l, p, cams, start, K, n) != 0 and f"{FWD}: invalid argument".encode() in l.mcnerf_last_error(), case
    assert _bwd(l, p, cams, start, K, n) != 0 and f"{BWD}: invalid argument".encode() in l.mcnerf_last_error(), case


@pytest.mark.parametrize("missing", FWD_PTRS + ["seg", "seed"])
def test_forward_refuses_null_pointers_without_a_gpu(missing):
    from mc_nerf_amd import _lib
    l = _lib.lib()
    p = ctypes.addressof(ctypes.create_string_buffer(4096))
    rc = _fwd(l, p, [0, 1], [0, 2, 4], 2, 4, seg=missing != "seg", draw=missing == "seed", missing=(missing,))
    assert rc != 0 and f"{FWD}: invalid argument".encode() in l.mcnerf_last_error(), missing


@pytest.mark.parametrize("missing", BWD_PTRS + ["seg"])
def test_backward_refuses_null_pointers_without_a_gpu(missing):
    from mc_nerf_amd import _lib
    l = _lib.lib()
    p = ctypes.addressof(ctypes.create_string_buffer(4096))
    rc = _bwd(l, p, [0, 1], [0, 2, 4], 2, 4, seg=missing != "seg", missing=(missing,))
    assert rc != 0 and f"{BWD}: invalid argument".encode() in l.mcnerf_last_error(), missing


def test_entry_points_refuse_bad_scalars_without_a_gpu():
    from mc_nerf_amd import _lib
    l = _lib.lib()
    p = ctypes.addressof(ctypes.create_string_buffer(4096))
    bad = lambda rc, name: rc != 0 and f"{name}: invalid argument".encode() in l.mcnerf_last_error()
    assert bad(_fwd(l, p, [0, 1], [0, 2, 4], 2, 4, channels=2), FWD)
    assert bad(_fwd(l, p, [0, 1], [0, 2, 4], 2, 4, H=0), FWD) and bad(_fwd(l, p, [0, 1], [0, 2, 4], 2, 4, W=0), FWD)
    assert bad(_fwd(l, p, [0, 1], [0, 17, 20], 2, 20, draw=True), FWD)          # a drawn segment longer than H W = 16
    assert bad(_bwd(l, p, [0, 1], [0, 2, 4], 2, 4, W=0), BWD)


def test_ops_refuse_cpu_tensors():
    from mc_nerf_amd import ops
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model.render import RayBatchFn
    s = R.make_case("b3")
    a = (s["pose"], s["kinv"], s["lens"], s["cams"], s["seg"])
    with pytest.raises(McnerfError):
        ops.lens_ray_batch_fwd(*a, s["H"], s["W"], pix=s["pix"])
    with pytest.raises(McnerfError):
        ops.lens_ray_batch_bwd(*a, s["W"], s["pix"], s["g_d"], s["g_o"])
    with pytest.raises(McnerfError):
        RayBatchFn.apply(s["pose"], s["kinv"], s["cams"], s["seg"], s["H"], s["W"], None, s["pix"], None, s["lens"])
    with pytest.raises(McnerfError):
        ops.lens_ray_batch_fwd(s["pose"], s["kinv"], s["lens"], s["cams"], s["seg"][:-1], s["H"], s["W"], pix=s["pix"])     # K + 1 entries


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_reference_distort_inverts_undistort():
    g = torch.Generator().manual_seed(0)
    xy = (torch.rand(4000, 2, generator=g, dtype=torch.float64) * 2 - 1) * 0.7                       # r_d <= 0.99
    lens = torch.stack([(torch.rand(4000, generator=g, dtype=torch.float64) * 2 - 1) * 0.08,
                        (torch.rand(4000, generator=g, dtype=torch.float64) * 2 - 1) * 0.01], -1)
    xy[0] = 0.0                                                                                       # the centre maps to itself
    for solve in ("implicit", "unrolled"):
        back = R.distort(R.undistort(xy, lens, solve), lens)
        assert float((back - xy).abs().max()) <= 1e-12, solve
    assert torch.equal(R.undistort(xy[:1], lens[:1]), xy[:1])
    # the library's own inverse (synthetic data generation) agrees with the restatement's
    from mc_nerf_amd import lens as L
    assert float((L.undistort_normalised(xy, lens) - R.undistort(xy, lens)).abs().max()) <= 1e-12


def test_reference_implicit_gradient_is_autograd_through_the_unrolled_solve():
    s = R.make_case("a3")
    a = (s["pose"], s["kinv"], s["lens"], s["cams"], s["seg"], s["pix"], s["W"])
    imp, unr = R.backward(*a, s["g_d"], s["g_o"]), R.backward(*a, s["g_d"], s["g_o"], solve="unrolled")
    for k in ("d_pose", "d_kinv", "d_lens"):
        assert float((imp[k] - unr[k]).abs().max()) <= 1e-12 * float(unr[k].abs().max()), k
        assert float((imp["terms"][k] - unr["terms"][k]).abs().max()) <= 1e-12 * float(unr["terms"][k].abs().max()), k
    assert float(imp["fprime"].min()) >= 0.5
    # and the kernel's formulas (the implicit derivative spelt out), evaluated in fp64, are the same per-ray terms
    t = R.kernel_terms(*a, s["g_d"], dtype=torch.float64)
    zero_o = R.backward(*a, s["g_d"], torch.zeros_like(s["g_o"]))
    for k, ref in (("d_lens", imp["terms"]["d_lens"]), ("d_kinv", imp["terms"]["d_kinv"]), ("d_R", zero_o["terms"]["d_pose"][:, :, :3])):
        assert float((t[k] - ref).abs().max()) <= 1e-11 * float(ref.abs().max()), k


def test_formulas_against_finite_differences_at_a_hand_worked_point():
    """k = (-0.1, 0) and the undistorted point (x_u, y_u) = (0.6, 0.8): r_u = 1, q = 1, D = 0.9, so the observed point is (0.54, 0.72),
    r_d = 0.9, s = 1 / 0.9, f' = 1 - 0.3 = 0.7.  ds/dk1 = -s q / f' = -1 / 0.63; ds/dk2 = -s q^2 / f' = -1 / 0.63;
    ds/d(x_d, y_d) = -s^3 (2 k1) / f' (x_d, y_d) = (0.2 / 0.5103) (0.54, 0.72)."""
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)
    xd, k = f64(0.54, 0.72), f64(-0.1, 0.0)

    def s_of(xy, kk):
        rd = xy.norm()
        return R.solve_radius(rd, kk[0], kk[1], "unrolled") / rd
    assert abs(float(s_of(xd, k)) - 1 / 0.9) <= 1e-14
    want_k, want_x = f64(-1 / 0.63, -1 / 0.63), (0.2 / 0.5103) * xd
    h = 1e-6
    for i in range(2):
        e = torch.zeros(2, dtype=torch.float64)
        e[i] = h
        fd_k = float(s_of(xd, k + e) - s_of(xd, k - e)) / (2 * h)
        fd_x = float(s_of(xd + e, k) - s_of(xd - e, k)) / (2 * h)
        assert abs(fd_k - float(want_k[i])) <= 1e-8 and abs(fd_x - float(want_x[i])) <= 1e-8, i
    xg, kg = xd.clone().requires_grad_(True), k.clone().requires_grad_(True)
    s_of(xg, kg).backward()
    assert torch.allclose(kg.grad, want_k, rtol=1e-12) and torch.allclose(xg.grad, want_x, rtol=1e-12)


def test_fp32_mode_runs_the_kernels_eight_steps():
    """At k = 0 the fp32 mode never moves r (s = 1 exactly); inside the test range it is within a few ulp of the fp64 root; for any
    finite k it stays finite and inside [0, 2 r_d]."""
    rd = torch.linspace(0.0, 1.0, 257)
    assert torch.equal(R.kernel_radius(rd, torch.zeros(257), torch.zeros(257)), rd)
    g = torch.Generator().manual_seed(1)
    k1, k2 = (torch.rand(257, generator=g) * 2 - 1) * 0.08, (torch.rand(257, generator=g) * 2 - 1) * 0.01
    exact = R.solve_radius(rd.double(), k1.double(), k2.double())
    assert float((R.kernel_radius(rd, k1, k2).double() - exact).abs().max()) <= 8 * 2.0 ** -24
    wild = R.kernel_radius(rd, (torch.rand(257, generator=g) * 2 - 1) * 50, (torch.rand(257, generator=g) * 2 - 1) * 50)
    assert bool(torch.isfinite(wild).all()) and bool((wild >= 0).all()) and bool((wild <= 2 * rd).all())


def test_margins_of_the_gpu_gates_are_what_the_cpu_measures():
    """M_F and M_B of tests/test_lens_gpu.py are 4 x the worst figure measured here, over all of that file's cases."""
    import test_lens_gpu as G
    m = {c: R.measure_margins(c) for c in R.CASES}
    fwd, bwd = max(v["fwd"] for v in m.values()), max(max(v["bwd"].values()) for v in m.values())
    print(f"[lens margins] fwd worst {fwd:.2f} units of 2^-24 (M_F = {G.M_F}), bwd worst {bwd:.2f} (M_B = {G.M_B})")
    assert 4 * fwd <= G.M_F <= 4 * fwd + 1 and 4 * bwd <= G.M_B <= 4 * bwd + 1
    assert min(v["min_fprime"] for v in m.values()) >= 0.5 and max(v["max_rd"] for v in m.values()) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ reprojection
def _reproj_case(dtype):
    g = torch.Generator().manual_seed(4)
    C, P = 3, 5
    K = torch.zeros(C, 3, 3, dtype=dtype)
    K[:, 0, 0], K[:, 1, 1] = 40 + 5 * torch.rand(C, generator=g, dtype=dtype), 38 + 5 * torch.rand(C, generator=g, dtype=dtype)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 26 + torch.rand(C, generator=g, dtype=dtype), 18 + torch.rand(C, generator=g, dtype=dtype), 1.0
    pix = torch.rand(1, C, P, 2, generator=g, dtype=dtype) * torch.tensor([53.0, 37.0], dtype=dtype)
    lens = torch.stack([(torch.rand(C, generator=g, dtype=dtype) * 2 - 1) * 0.08, (torch.rand(C, generator=g, dtype=dtype) * 2 - 1) * 0.01], -1)
    return pix, K, lens


def test_reprojection_op_is_the_identity_at_zero_and_the_forward_model_otherwise():
    from mc_nerf_amd.lens import distort_pixels
    pix, K, lens = _reproj_case(torch.float32)
    assert torch.equal(distort_pixels(pix, K, torch.zeros_like(lens)), pix)
    pix, K, lens = _reproj_case(torch.float64)
    got = distort_pixels(pix, K, lens)
    f, c = torch.stack([K[:, 0, 0], K[:, 1, 1]], -1)[:, None], torch.stack([K[:, 0, 2], K[:, 1, 2]], -1)[:, None]
    want = R.distort((pix - c) / f, lens[:, None]) * f + c
    assert float((got - want).abs().max()) <= 1e-12 * 53 and float((got - pix).abs().max()) > 1e-2


def test_reprojection_op_gradients_pass_gradcheck():
    from mc_nerf_amd.lens import distort_pixels
    pix, K, lens = _reproj_case(torch.float64)
    # K enters through its four intrinsic entries only: check the gradient with respect to those
    def f(pix, fx, fy, cx, cy, lens):
        Km = torch.zeros(3, 3, 3, dtype=torch.float64)
        Km[:, 0, 0], Km[:, 1, 1], Km[:, 0, 2], Km[:, 1, 2], Km[:, 2, 2] = fx, fy, cx, cy, 1.0
        return distort_pixels(pix, Km, lens)
    leaves = [t.clone().requires_grad_(True) for t in (pix, K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], lens)]
    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-7, rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ the model
def _cpu_step(model, sp, stage, cam=3):
    from mc_nerf_amd.model import MC_NeRF_Loss
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0], lens=S.lens_distortion(sp["data_numb"][0], 2))
    model.get_rays = lambda pose, img_id, intr_inv: (torch.zeros(64, 3), torch.zeros(64, 3))      # (validation rays: HIP only)
    data = (torch.zeros(1, 64, 3), torch.tensor([cam]), wpts, pts, wpts, pts)
    loss_dict, *_ = model(data, 0, stage, 0.0)
    return MC_NeRF_Loss(sp)(loss_dict, stage)


def test_camera_only_stage_of_a_cpu_model_reaches_the_lens_parameter():
    m, sp = _model(lens_model="radial")
    S.init_cameras_near_gt(m, noise=0.01)
    loss = _cpu_step(m, sp, "CAM_PARAM_EPOCH")
    loss.backward()
    g = m.weights_lens.grad
    assert bool(torch.isfinite(loss)) and g is not None and g.shape == m.weights_lens.shape
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert m.weights_fx.grad is not None and float(m.weights_fx.grad.abs().max()) > 0
    # at weights_lens = 0 the reprojected pixels are the pinhole model's bits
    base, _ = _model()
    S.init_cameras_near_gt(base, noise=0.01)
    wpts, _ = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    outs = []
    for mod in (m, base):
        intr, pose, calib = mod.add_weights2param(True, True, True, wpts, wpts)
        outs.append(mod._reproject(wpts, intr, calib, 0))
    assert torch.equal(outs[0], outs[1])


def test_nerf_stage_of_a_cpu_model_raises():
    from mc_nerf_amd._lib import McnerfError
    m, sp = _model(lens_model="radial")
    with pytest.raises(McnerfError):
        _cpu_step(m, sp, "GLOBAL_OPTIM_EPOCH")
    m, sp = _model(lens_model="radial", cams_per_step=2)
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    with pytest.raises(McnerfError):
        m((torch.zeros(2, 64, 3), torch.tensor([1, 4]), wpts, pts, wpts, pts), 0, "GLOBAL_OPTIM_EPOCH", 0.0)


# ------------------------------------------------------------------------------------------------------------------ synthetic data
def test_synthetic_defaults_are_todays_outputs():
    pose, K, _ = S.ball_cameras(0, H=8, W=8)
    a, b = S.calibration_points(pose, K, seed=3), S.calibration_points(pose, K, seed=3, lens=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    z = S.calibration_points(pose, K, seed=3, lens=torch.zeros(pose.shape[0], 2))
    assert torch.equal(z[0], a[0]) and float((z[1] - a[1]).abs().max()) <= 1e-5              # (through fp64 and back)
    lens = S.lens_distortion(pose.shape[0], seed=1, k1_spread=0.05, k2_spread=0.005)
    assert lens.shape == (pose.shape[0], 2) and torch.equal(lens, S.lens_distortion(pose.shape[0], seed=1, k1_spread=0.05, k2_spread=0.005))
    assert 0.02 < float(lens[:, 0].std()) < 0.08 and 0.002 < float(lens[:, 1].std()) < 0.008
    d = S.calibration_points(pose, K, seed=3, lens=lens)
    assert torch.equal(d[0], a[0]) and float((d[1] - a[1]).abs().max()) > 1e-3
    import inspect
    assert inspect.signature(S.blob_scene_images).parameters["lens"].default is None
    # the fp64 rays of a distorted camera: at k = 0 the pinhole restatement, otherwise the restatement with the lens
    import multicam_ref as MR
    pix = torch.arange(64)
    d0, o0 = S.lens_rays(pose[5], K[5], torch.zeros(2), 8, 8)
    kinv = torch.linalg.inv(K.double())
    want_d, want_o = MR.rays(pose, kinv, [5], [0, 64], pix, 8)
    assert float((d0.double() - want_d).abs().max()) <= 1e-6 and float((o0.double() - want_o).abs().max()) <= 1e-6
    d1, _ = S.lens_rays(pose[5], K[5], lens[5], 8, 8)
    want_d1 = R.rays(pose, kinv, lens, [5], [0, 64], pix, 8)[0]
    assert float((d1.double() - want_d1).abs().max()) <= 1e-6 and float((d1 - d0).abs().max()) > 1e-4


# ------------------------------------------------------------------------------------------------------------------ plumbing
def test_flat_grad_sync_and_radam_carry_the_lens_parameter_like_any_camera_parameter():
    from mc_nerf_amd.distributed import FlatGradSync
    from mc_nerf_amd.model import RAdam
    m, sp = _model(lens_model="radial")
    base, _ = _model()
    a, b = FlatGradSync(m, 1), FlatGradSync(base, 1)
    assert any(p is m.weights_lens for p in a.cam_params) and len(a.cam_params) == len(b.cam_params) + 1
    assert a.n_grad == b.n_grad + 2 * sp["data_numb"][0] and a.n_flags == b.n_flags + 1
    opt = RAdam([{"params": [p for n, p in m.named_parameters() if n != "weights_lens"]},
                 {"params": [m.weights_lens], "betas": (0.0, 0.999), "lr": 1e-3}], lr=5e-4)
    m.weights_lens.grad = torch.full_like(m.weights_lens, 0.5)
    opt.step()
    assert torch.allclose(m.weights_lens.detach(), torch.full_like(m.weights_lens, -0.5e-3))
