"""The per-camera colour calibration (`color_calib`) without a GPU: the entry point in the header, the ctypes table and
the built library; the sys_param keys at model construction; the eager loss of host tensors against the fp64 restatement
(tests/color_calib_ref.py); the op's refusal of CPU tensors and the C entry point's refusal of a bad segment table ahead of any
device work; the restatement itself on a case worked by hand."""
import ctypes
import os
import re

import pytest
import torch

import color_calib_ref as R
from mc_nerf_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mcnerf_train_loss_calib"


def _model(**kw):
    from mc_nerf_amd.model import MC_Model
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    sp.update(kw)
    return MC_Model(sp), sp


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_declares_the_calibrated_loss_and_keeps_its_version():
    from mc_nerf_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, "include", "mcnerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "color_calib.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "color_calib.hip"))
    assert "mcnerf_colorcal.h" in build.HEADERS and os.path.isfile(os.path.join(build.CSRC, "mcnerf_colorcal.h"))
    lib = ctypes.CDLL(build.build(verbose=False))
    assert f"int {NAME}(" in code and hasattr(lib, NAME)
    assert _lib.ABI_VERSION == 7                             # (new symbols only; tests/test_abi_cpu.py checks header, table and library)
    assert f"#define MCNERF_TRAIN_LOSS_CALIB_OUT {ops.TRAIN_LOSS_CALIB_OUT}\n" in hdr
    assert f"#define MCNERF_TRAIN_LOSS_CALIB_WS {ops.TRAIN_LOSS_CALIB_WS}\n" in hdr


def test_digested_kernel_sources_do_not_include_the_new_files():
    """The loss kernel lives outside the sources whose digest ties the recorded MLP-kernel traffic to the code."""
    import bench
    assert "color_calib.hip" not in bench.MLP_KERNEL_SOURCES and "mcnerf_colorcal.h" not in bench.MLP_KERNEL_SOURCES
    csrc = os.path.join(ROOT, "mc_nerf_amd", "csrc")
    for f in bench.MLP_KERNEL_SOURCES:
        assert "colorcal" not in open(os.path.join(csrc, f)).read(), f


# ------------------------------------------------------------------------------------------------------------------ the keys
@pytest.mark.parametrize("bad", ["gain", "Affine", True, 1, None, ""])
def test_bad_color_calib_is_refused(bad):
    with pytest.raises(ValueError, match="color_calib"):
        _model(color_calib=bad)


@pytest.mark.parametrize("bad", [-1e-3, -1, float("nan"), float("inf"), "1e-3", None, True])
def test_bad_color_calib_reg_is_refused(bad):
    with pytest.raises(ValueError, match="color_calib_reg"):
        _model(color_calib="affine", color_calib_reg=bad)
    from mc_nerf_amd.model import MC_NeRF_Loss
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    sp["color_calib_reg"] = bad
    with pytest.raises(ValueError, match="color_calib_reg"):
        MC_NeRF_Loss(sp)


@pytest.mark.parametrize("kw", [{}, {"color_calib": "none"}])
def test_default_model_has_the_46_keys_and_no_colour_parameter(kw):
    m, _ = _model(**kw)
    sd = m.state_dict()
    assert len(sd) == 46 and not any("weights_color" in k for k in sd) and not hasattr(m, "weights_color")
    with pytest.raises(ValueError, match="color_calib"):
        m.color_correction()


def test_affine_model_adds_one_zero_parameter():
    m, sp = _model(color_calib="affine", color_calib_reg=0)
    base, _ = _model()
    C = sp["data_numb"][0]
    sd = m.state_dict()
    assert len(sd) == 47 and set(sd) - set(base.state_dict()) == {"weights_color"}
    assert m.weights_color.shape == (C, 6) and m.weights_color.requires_grad and torch.equal(m.weights_color.detach(), torch.zeros(C, 6))
    g, b = m.color_correction()
    assert torch.equal(g, torch.ones(C, 3)) and torch.equal(b, torch.zeros(C, 3)) and not g.requires_grad and not b.requires_grad
    assert m.color_calib_reg == 0.0 and _model(color_calib="affine")[0].color_calib_reg == 1e-3
    # the renderer's checkpoint filter does not see the new key
    from mc_nerf_amd.model import NeRF_Model
    for coarse in (True, False):
        assert set(NeRF_Model.rewrite_nerf_ckpt({"model_nerf": sd}, coarse=coarse)) == set(NeRF_Model.rewrite_nerf_ckpt({"model_nerf": base.state_dict()}, coarse=coarse))


# ------------------------------------------------------------------------------------------------------------------ eager loss
def _case(n, cams, C, with_fine, seed=0):
    from mc_nerf_amd import ops
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=gen)
    return dict(rgb_c=r(n, 3), rgb_f=r(n, 3) if with_fine else None, gt=r(n, 3), color_w=0.6 * r(C, 6) - 0.3, cams=list(cams),
                seg_start=ops.ray_segments(n, len(cams)), pd=8 * r(1, C, 5, 2), pt_gt=8 * r(1, C, 5, 2))


@pytest.mark.parametrize("with_fine", [True, False])
@pytest.mark.parametrize("epoch_type", ["GLOBAL_OPTIM_EPOCH", "CAM_PARAM_EPOCH"])
def test_eager_loss_of_host_tensors_matches_the_fp64_restatement(with_fine, epoch_type):
    from mc_nerf_amd.model import MC_NeRF_Loss
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    sp["color_calib_reg"] = 0.25
    loss_fn = MC_NeRF_Loss(sp)
    c = _case(23, [3, 0, 3, 5], 7, with_fine)
    normalise = epoch_type != "CAM_PARAM_EPOCH"
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    pd, rc, rf, w = leaf(c["pd"]), leaf(c["rgb_c"]), leaf(c["rgb_f"]), leaf(c["color_w"])
    total = loss_fn({"intr": [pd, c["pt_gt"]], "rgb": [rc, rf, c["gt"]], "color": [w, c["cams"], c["seg_start"]]}, epoch_type)
    total.backward()
    ref = R.grads(c["pd"], c["pt_gt"], 8, 8, normalise, c["rgb_c"], c["rgb_f"], c["gt"], c["color_w"], c["cams"], c["seg_start"], 0.25)
    assert abs(float(total.detach()) - float(ref["value"])) <= 1e-6 * abs(float(ref["value"]))
    for got, key in ((pd.grad, "d_pd"), (rc.grad, "d_c"), (w.grad, "d_color")) + (((rf.grad, "d_f"),) if with_fine else ()):
        assert float((got.double() - ref[key]).abs().max()) <= 1e-6 * float(ref[key].abs().max()), key
    assert float(w.grad[[1, 2, 4, 6]].abs().max()) == 0.0             # cameras outside the step
    # the stand-alone form: no reprojection term, an explicit reg
    alone = loss_fn.get_rgb_loss_calibrated([c["rgb_c"], c["rgb_f"], c["gt"]], c["color_w"], c["cams"], c["seg_start"], reg=0.5)
    want = R.loss(None, None, 8, 8, False, c["rgb_c"], c["rgb_f"], c["gt"], c["color_w"], c["cams"], c["seg_start"], 0.5)["total"]
    assert abs(float(alone) - float(want)) <= 1e-6 * float(want)


@pytest.mark.parametrize("with_fine", [True, False])
def test_eager_loss_at_identity_is_the_plain_rgb_loss(with_fine):
    from mc_nerf_amd.model import MC_NeRF_Loss
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    loss_fn = MC_NeRF_Loss(sp)
    c = _case(23, [3, 0, 3, 5], 7, with_fine)
    rgbs = [c["rgb_c"], c["rgb_f"], c["gt"]]
    assert torch.equal(loss_fn.get_rgb_loss_calibrated(rgbs, torch.zeros(7, 6), c["cams"], c["seg_start"], reg=0.0), loss_fn.get_rgb_loss(rgbs))
    with pytest.raises(ValueError, match="color_calib_reg"):
        loss_fn.get_rgb_loss_calibrated(rgbs, torch.zeros(7, 6), c["cams"], c["seg_start"], reg=-1.0)


def test_plain_keys_keep_their_path():
    """{"intr", "rgb"} on host tensors: the eager total of before, whatever the colour keys say."""
    from mc_nerf_amd.model import MC_NeRF_Loss
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    c = _case(23, [3, 0, 3, 5], 7, True)
    d = {"intr": [c["pd"], c["pt_gt"]], "rgb": [c["rgb_c"], c["rgb_f"], c["gt"]]}
    a = MC_NeRF_Loss(sp)(d, "GLOBAL_OPTIM_EPOCH")
    sp2 = dict(sp, color_calib="affine", color_calib_reg=3.0)
    assert torch.equal(MC_NeRF_Loss(sp2)(d, "GLOBAL_OPTIM_EPOCH"), a)


def test_flat_grad_sync_carries_the_colour_parameter_like_any_camera_parameter():
    """distributed.FlatGradSync takes every non-`nerf.` parameter as a dense camera gradient: nothing special for weights_color."""
    from mc_nerf_amd.distributed import FlatGradSync
    m, sp = _model(color_calib="affine")
    base, _ = _model()
    a, b = FlatGradSync(m, 1), FlatGradSync(base, 1)
    assert any(p is m.weights_color for p in a.cam_params) and len(a.cam_params) == len(b.cam_params) + 1
    assert a.n_grad == b.n_grad + 6 * sp["data_numb"][0] and a.n_flags == b.n_flags + 1


def test_radam_groups_with_betas_of_their_own_get_their_own_step_sizes():
    """A camera group without momentum (betas (0, 0.999)) beside the nets' group: the step-size cache is per group, so the group's
    first steps use 1 / (1 - 0^t) = 1, not the other group's 1 / (1 - 0.9^t) = 10, 5.26, 3.69; one group alone is as before."""
    from mc_nerf_amd.model import RAdam
    a, b, c = (torch.nn.Parameter(torch.ones(3)) for _ in range(3))
    two = RAdam([{"params": [a]}, {"params": [b], "betas": (0.0, 0.999)}], lr=1e-2)
    one = RAdam([c], lr=1e-2)
    assert two.param_groups[0]["buffer"] is not two.param_groups[1]["buffer"]
    for t in range(1, 4):
        for p in (a, b, c):
            p.grad = torch.full((3,), 0.5)
        two.step()
        one.step()
        assert two.param_groups[1]["buffer"][t % 10][2] == 1.0
        assert abs(two.param_groups[0]["buffer"][t % 10][2] - 1.0 / (1.0 - 0.9 ** t)) < 1e-12
        assert torch.equal(a.detach(), c.detach())                 # the first group steps as a lone group does
        assert torch.allclose(b.detach(), torch.full((3,), 1.0 - t * 1e-2 * 0.5))      # un-rectified steps: p -= lr * 1 * grad
    two.add_param_group({"params": [torch.nn.Parameter(torch.ones(1))]})
    assert two.param_groups[2]["buffer"] is not two.param_groups[0]["buffer"]


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_op_refuses_cpu_tensors():
    from mc_nerf_amd import ops
    from mc_nerf_amd._lib import McnerfError
    c = _case(6, [1, 2], 4, True)
    with pytest.raises(McnerfError):
        ops.train_loss_calib(c["pd"], c["pt_gt"], 8, 8, True, c["rgb_c"], c["rgb_f"], c["gt"], c["color_w"], [1, 2], [0, 3, 6], 1e-3)
    with pytest.raises(McnerfError):
        ops.train_loss_calib(None, None, 8, 8, False, c["rgb_c"], None, c["gt"], c["color_w"], [1, 2], [0, 3], 1e-3)      # K + 1 entries


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


def _call(l, p, cams, start, K, n, *, reg=1e-3, rgb_c=True, gt=True, color_w=True, out=True, d_c=True, d_f=True, d_color=True, partials=True,
          seg=True, np_=0):
    q = lambda on: p if on else None
    return l.mcnerf_train_loss_calib(None, None, np_, 4, 4, 1, q(rgb_c), p, q(gt), n, q(color_w), 7, _i32(cams) if seg else None,
                                     _i32(start) if seg else None, K, reg, q(out), None, q(d_c), q(d_f), q(d_color), q(partials), None)


@pytest.mark.parametrize("case", sorted(BAD_TABLES))
def test_entry_point_refuses_a_bad_segment_table_without_a_gpu(case):
    """The refusals sit ahead of any HIP call: non-zero on a machine without a GPU.  The device pointers are never read: a host
    buffer stands in for them."""
    from mc_nerf_amd import _lib
    l = _lib.lib()
    cams, start, K, n = BAD_TABLES[case]
    buf = ctypes.create_string_buffer(4096)
    rc = _call(l, ctypes.addressof(buf), cams, start, K, n)
    assert rc != 0 and b"mcnerf_train_loss_calib: invalid argument" in l.mcnerf_last_error(), case


@pytest.mark.parametrize("missing", ["rgb_c", "gt", "color_w", "out", "d_c", "d_f", "d_color", "partials", "seg"])
def test_entry_point_refuses_null_pointers_without_a_gpu(missing):
    from mc_nerf_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    rc = _call(l, ctypes.addressof(buf), [0, 1], [0, 2, 4], 2, 4, **{missing: False})
    assert rc != 0 and b"mcnerf_train_loss_calib: invalid argument" in l.mcnerf_last_error(), missing


def test_entry_point_refuses_bad_scalars_without_a_gpu():
    from mc_nerf_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert _call(l, p, [0, 1], [0, 2, 4], 2, 4, reg=-1.0) != 0 and b"invalid argument" in l.mcnerf_last_error()
    assert _call(l, p, [0], [0, 0], 1, 0) != 0 and b"invalid argument" in l.mcnerf_last_error()               # no rays
    assert _call(l, p, [0, 1], [0, 2, 4], 2, 4, np_=3) != 0 and b"invalid argument" in l.mcnerf_last_error()   # points without pd


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_fp64_reference_on_a_case_worked_by_hand():
    """3 rays, 2 cameras, table ([1, 0], [0, 2, 3]), coarse render only, reg = 0.9.  Camera 1 is the identity; camera 0 has gain
    (2, 1, 1) and bias (0, 0, 0.5).  Residuals: ray 0 (1, 0, 0), ray 1 zero, ray 2 (2 * 0.5 - 0, 0.5 - 0.5, 0.5 + 0.5 - 0) =
    (1, 0, 1): L_rgb = 3 / 9.  L_reg = 0.9 / 2 * (0 + (1 + 0.25) / 6) = 0.09375.  With gr = 2 / 9: d_c of ray 2 = gr e g =
    (4/9, 0, 2/9); row 0 of d_color = (gr e rgb | gr e) of ray 2 + 0.15 w = (1/9 + 0.15, 0, 1/9, 2/9, 0, 2/9 + 0.075); row 1 =
    (2/9, 0, 0, 2/9, 0, 0) from ray 0."""
    w = torch.tensor([[1.0, 0, 0, 0, 0, 0.5], [0, 0, 0, 0, 0, 0]])
    rgb = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0.5, 0.5, 0.5]])
    gt = torch.tensor([[0.0, 0, 0], [0, 1.0, 0], [0, 0.5, 0]])
    r = R.grads(None, None, 4, 4, True, rgb, None, gt, w, [1, 0], [0, 2, 3], 0.9)
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)
    assert torch.allclose(r["l_rgb"], f64(1 / 3), rtol=1e-14) and torch.allclose(r["l_reg"], f64(0.09375), rtol=1e-14)
    assert torch.allclose(r["value"], f64(1 / 3 + 0.09375), rtol=1e-14) and float(r["l_intr"]) == 0.0
    assert torch.allclose(r["d_c"], f64([[2 / 9, 0, 0], [0, 0, 0], [4 / 9, 0, 2 / 9]]), rtol=1e-14, atol=0)
    want = f64([[1 / 9 + 0.15, 0, 1 / 9, 2 / 9, 0, 2 / 9 + 0.075], [2 / 9, 0, 0, 2 / 9, 0, 0]])
    assert torch.allclose(r["d_color"], want, rtol=1e-14, atol=0)
    assert torch.allclose(r["abs_sum"]["d_color"], want, rtol=1e-14, atol=0) and r["d_f"] is None and r["d_pd"] is None
    # an upstream factor scales every gradient and the magnitudes; an empty segment adds nothing, its camera's row stays zero
    r2 = R.grads(None, None, 4, 4, True, rgb, None, gt, w, [1, 0], [0, 2, 3], 0.9, upstream=-0.5)
    assert torch.allclose(r2["d_color"], -0.5 * want, rtol=1e-14) and torch.allclose(r2["abs_sum"]["d_color"], 0.5 * want, rtol=1e-14)
    r3 = R.grads(None, None, 4, 4, True, rgb, None, gt, torch.cat([w, torch.ones(1, 6)]), [1, 2, 0], [0, 2, 2, 3], 0.9)
    assert float(r3["d_color"][2].abs().max()) == 0.0 and torch.allclose(r3["l_reg"], f64(0.09375 * 2 / 3), rtol=1e-14)
    # mixed signs: the magnitudes exceed the cancelled sum
    r4 = R.grads(None, None, 4, 4, True, rgb, gt, rgb.flip(0), w, [1, 0], [0, 2, 3], 0.0)
    assert bool((r4["abs_sum"]["d_color"] >= r4["d_color"].abs() - 1e-15).all()) and float(r4["abs_sum"]["d_color"][1, 3]) > float(r4["d_color"][1, 3].abs()) + 0.1
