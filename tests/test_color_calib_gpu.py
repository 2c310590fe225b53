"""The per-camera colour calibration (`color_calib` = "affine"; csrc/color_calib.hip) on the GPU.

The fused loss is gated against the fp64 restatement of tests/color_calib_ref.py: value, d_pd, d_c, d_f at the bars of
test_a_ops_gpu.py::test_fused_train_loss_matches_eager_formulation (2e-6 of the largest entry), d_color -- a sum of mixed signs over
a camera's rays -- at the same 2e-6 taken on the sum of the magnitudes that were added.  At weights_color = 0 the ray gradients are
the bits of mcnerf_train_loss; two runs are the same bits; the model step carries the new loss key and trains the new parameter.

Shapes (H, W = 12, 20; C = 11), the smallest at which each indexing rule can go wrong:
  n1      1 ray, 1 segment;
  n5      5 rays, 3 segments of 2, 2, 1 rays;
  n64     64 rays, 64 segments of one ray (the longest table), C = 70;
  n7001   7001 rays, cameras [3, 0, 3, 9, 1, 0, 5] of 11: ragged segments (one of a single ray), two cameras twice, five absent; 4 blocks
          per segment;
  n70001  70 001 rays, 5 segments: 25 blocks per segment, every block grid-strides more than once;
  empty   300 rays, 4 segments of which one is empty (it adds nothing; its camera's row stays zero)."""
import math
import os

import pytest
import torch

import color_calib_ref as R
from mc_nerf_amd import synthetic as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 12, 20
UPSTREAM = 0.37
REG = 0.05
SHAPES = {                           # n, cameras, seg_start (None: ops.ray_segments), C
    "n1": (1, [4], None, 11),
    "n5": (5, [7, 2, 10], None, 11),
    "n64": (64, None, None, 70),
    "n7001": (7001, [3, 0, 3, 9, 1, 0, 5], [0, 1500, 1501, 2800, 3303, 5000, 6100, 7001], 11),
    "n70001": (70001, [6, 1, 8, 0, 2], None, 11),
    "empty": (300, [2, 5, 2, 7], [0, 100, 100, 250, 300], 11),
}


@pytest.fixture(scope="module")
def cases(gpu_device):
    """Per shape: the step's tensors on the host (the restatement reads them) and on the device -- made once, shared, never written to."""
    from mc_nerf_amd import ops
    out = {}
    for i, (name, (n, cams, seg, C)) in enumerate(SHAPES.items()):
        g = torch.Generator().manual_seed(100 + i)
        if cams is None:
            cams = torch.randperm(C, generator=g)[:n].tolist()
        seg = ops.ray_segments(n, len(cams)) if seg is None else seg
        host = dict(rgb_c=torch.rand(n, 3, generator=g), rgb_f=torch.rand(n, 3, generator=g), gt=torch.rand(n, 3, generator=g),
                    color_w=0.6 * torch.rand(C, 6, generator=g) - 0.3, pd=float(W) * torch.rand(1, C, 5, 2, generator=g))
        host["pt_gt"] = host["pd"] + torch.randn(1, C, 5, 2, generator=g)
        out[name] = dict(n=n, cams=cams, seg=seg, C=C, host=host, dev={k: v.to(gpu_device) for k, v in host.items()})
    return out


def _record(name, text):
    """profiles/color_calib_parity.txt: one line per case, rewritten by every run of the parity test."""
    path = os.path.join(ROOT, "profiles", "color_calib_parity.txt")
    head = ("# mcnerf_train_loss_calib (csrc/color_calib.hip) against the fp64 restatement tests/color_calib_ref.py: the worst ratio\n"
            "# |d_color - ref| / abs_sum over the entries of d_color (gate 2e-6) and the relative error of the value (gate 2e-6);\n"
            "# written by tests/test_color_calib_gpu.py::test_op_matches_the_fp64_restatement\n")
    try:
        lines = {}
        if os.path.isfile(path):
            lines = {l.split(":")[0]: l for l in open(path).read().splitlines() if l and not l.startswith("#")}
        lines[name] = f"{name}: {text}"
        with open(path, "w") as f:
            f.write(head + "\n".join(lines[k] for k in sorted(lines)) + "\n")
    except OSError:                     # (a read-only checkout: the figures are still printed)
        pass


def _run_fn(c, normalise, with_fine, reg=REG, upstream=UPSTREAM):
    """TrainLossCalibFn on the case's device tensors, backward with the upstream factor -> (value, d_pd, d_c, d_f, d_color)."""
    from mc_nerf_amd.model.render import TrainLossCalibFn
    d = c["dev"]
    leaf = lambda t: t.clone().requires_grad_(True)
    pd, rc, rf, w = leaf(d["pd"]), leaf(d["rgb_c"]), leaf(d["rgb_f"]) if with_fine else None, leaf(d["color_w"])
    total = TrainLossCalibFn.apply(pd, d["pt_gt"], rc, rf, d["gt"], w, c["cams"], c["seg"], H, W, normalise, reg)
    (upstream * total).backward()
    return total.detach(), pd.grad, rc.grad, None if rf is None else rf.grad, w.grad


def _check_against_ref(got, ref, C, cams, label):
    """Gate 1 of the issue on (value, d_pd, d_c, d_f, d_color); -> (worst d_color ratio, relative value error)."""
    value, d_pd, d_c, d_f, d_color = got
    v_ref = float(ref["value"])
    v_err = abs(float(value) - v_ref) / max(1.0, abs(v_ref))
    print(f"[color calib, {label}] value {float(value):.9g} ref {v_ref:.9g} rel err {v_err:.2e}")
    assert v_err <= 2e-6, label
    for name, g in (("d_pd", d_pd), ("d_c", d_c), ("d_f", d_f)):
        if g is None:
            assert ref[name] is None
            continue
        err, big = float((g.cpu().double() - ref[name]).abs().max()), float(ref[name].abs().max())
        print(f"[color calib, {label}] {name} err {err:.3e} max|ref| {big:.3e}")
        assert err <= 2e-6 * big + 1e-12, (label, name)
    err = (d_color.cpu().double() - ref["d_color"]).abs()
    bound = 2e-6 * ref["abs_sum"]["d_color"] + 1e-12
    ratio = float((err / (ref["abs_sum"]["d_color"] + 1e-300)).max())
    print(f"[color calib, {label}] d_color worst |err| / abs_sum {ratio:.3e} (gate 2e-6)")
    assert bool((err <= bound).all()), (label, ratio)
    absent = [c for c in range(C) if c not in cams]
    if absent:
        assert float(d_color[absent].abs().max()) == 0.0, label
    return ratio, v_err


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("with_fine", [True, False])
@pytest.mark.parametrize("normalise", [True, False])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_op_matches_the_fp64_restatement(cases, shape, normalise, with_fine):
    c = cases[shape]
    h = c["host"]
    got = _run_fn(c, normalise, with_fine)
    ref = R.grads(h["pd"], h["pt_gt"], H, W, normalise, h["rgb_c"], h["rgb_f"] if with_fine else None, h["gt"], h["color_w"], c["cams"],
                  c["seg"], REG, upstream=UPSTREAM)
    label = f"{shape} normalise={int(normalise)} fine={int(with_fine)}"
    ratio, v_err = _check_against_ref(got, ref, c["C"], c["cams"], label)
    assert all(float(ref["abs_sum"]["d_color"][cam].min()) > 0 for cam, a, b in zip(c["cams"], c["seg"], c["seg"][1:]) if b > a)
    if shape == "empty":
        assert float(got[4][5].abs().max()) == 0.0                   # the camera of the empty segment
    _record(label, f"d_color worst |err| / abs_sum {ratio:.3e}, value rel err {v_err:.2e}")


def test_parts_of_the_value(cases):
    """out[0..3] = total, L_intr, L_rgb, L_reg."""
    from mc_nerf_amd import ops
    c = cases["n7001"]
    d, h = c["dev"], c["host"]
    out, *_ = ops.train_loss_calib(d["pd"], d["pt_gt"], H, W, True, d["rgb_c"], d["rgb_f"], d["gt"], d["color_w"], c["cams"], c["seg"], REG)
    ref = R.loss(h["pd"], h["pt_gt"], H, W, True, h["rgb_c"], h["rgb_f"], h["gt"], h["color_w"], c["cams"], c["seg"], REG)
    for i, key in enumerate(("total", "l_intr", "l_rgb", "l_reg")):
        assert abs(float(out[i]) - float(ref[key])) <= 2e-6 * max(1.0, abs(float(ref[key]))), key
    assert float(ref["l_reg"]) > 1e-4 and abs(float(out[3]) - float(ref["l_reg"])) <= 2e-6 * float(ref["l_reg"])


# ------------------------------------------------------------------------------------------------------------------ 2. identity
@pytest.mark.parametrize("with_fine", [True, False])
@pytest.mark.parametrize("shape", ["n5", "n7001", "n70001"])
def test_zero_weights_give_the_plain_loss_kernels_ray_gradients_bit_for_bit(cases, shape, with_fine):
    from mc_nerf_amd import ops
    c = cases[shape]
    d = c["dev"]
    rf = d["rgb_f"] if with_fine else None
    out0, p0, c0, f0 = ops.train_loss(d["pd"], d["pt_gt"], H, W, True, d["rgb_c"], rf, d["gt"])
    out1, p1, c1, f1, dw = ops.train_loss_calib(d["pd"], d["pt_gt"], H, W, True, d["rgb_c"], rf, d["gt"], torch.zeros_like(d["color_w"]),
                                                c["cams"], c["seg"], 0.0)
    assert torch.equal(c1, c0) and (f0 is None and f1 is None or torch.equal(f1, f0))
    assert abs(float(out1[0]) - float(out0[0])) <= 2e-6 * abs(float(out0[0]))                 # (another summation order)
    assert float((p1 - p0).abs().max()) <= 2e-6 * float(p0.abs().max())
    assert float(out1[3]) == 0.0 and bool(torch.isfinite(dw).all())


def test_host_tensor_beside_device_renders_is_refused_before_any_launch(cases):
    from mc_nerf_amd import ops
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import MC_NeRF_Loss
    c = cases["n5"]
    d, h = c["dev"], c["host"]
    for swap in ("color_w", "gt", "rgb_f", "pd"):
        a = dict(d, **{swap: h[swap]})
        with pytest.raises(McnerfError, match=swap):
            ops.train_loss_calib(a["pd"], a["pt_gt"], H, W, True, a["rgb_c"], a["rgb_f"], a["gt"], a["color_w"], c["cams"], c["seg"], REG)
    with pytest.raises(McnerfError, match="color_w"):
        ops.train_loss_calib(d["pd"], d["pt_gt"], H, W, True, d["rgb_c"], d["rgb_f"], d["gt"], d["color_w"].double(), c["cams"], c["seg"], REG)
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=H, W=W, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    with pytest.raises(McnerfError, match="color_w"):          # a parameter created on the CPU
        MC_NeRF_Loss(sp).get_rgb_loss_calibrated([d["rgb_c"], d["rgb_f"], d["gt"]], torch.nn.Parameter(torch.zeros(c["C"], 6)), c["cams"], c["seg"])


# ------------------------------------------------------------------------------------------------------------------ 3. determinism
def test_two_runs_are_the_same_bits_and_the_counter_is_left_at_zero(cases, gpu_device):
    from mc_nerf_amd import ops
    c = cases["n7001"]
    d = c["dev"]
    buf = torch.zeros(ops.TRAIN_LOSS_CALIB_OUT + ops.TRAIN_LOSS_CALIB_WS, dtype=torch.float32, device=gpu_device)
    run = lambda out=None: ops.train_loss_calib(d["pd"], d["pt_gt"], H, W, True, d["rgb_c"], d["rgb_f"], d["gt"], d["color_w"], c["cams"], c["seg"],
                                                REG, out=out)
    a = [t.clone() for t in run(buf)]
    assert int(buf[4].view(torch.int32)) == 0
    b = [t.clone() for t in run(buf)]
    assert int(buf[4].view(torch.int32)) == 0
    third = [t.clone() for t in run(buf)]                            # the same `out` buffer a third time
    fresh = run()
    for x, y, z, f in zip(a, b, third, fresh):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, f)


# ------------------------------------------------------------------------------------------------------------------ 4. K = 1
@pytest.mark.parametrize("shape", ["n5", "n7001"])
def test_one_segment_is_the_eager_formula_with_one_camera_for_all_rays(cases, shape):
    """The table ([c], [0, n]) of a single-camera step against the eager formulation of MC_NeRF_Loss on host tensors."""
    from mc_nerf_amd import ops
    from mc_nerf_amd.model import MC_NeRF_Loss
    c = cases[shape]
    d, h, n, cam = c["dev"], c["host"], c["n"], 9
    out, d_pd, d_c, d_f, d_w = ops.train_loss_calib(d["pd"], d["pt_gt"], H, W, True, d["rgb_c"], d["rgb_f"], d["gt"], d["color_w"], [cam], [0, n], REG)
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=H, W=W, coarse=(4, 32, [2]), fine=(8, 64, [4]), color_calib_reg=REG)
    leaf = lambda t: t.clone().requires_grad_(True)
    pd, rc, rf, w = leaf(h["pd"]), leaf(h["rgb_c"]), leaf(h["rgb_f"]), leaf(h["color_w"])
    g, b = 1.0 + w[cam, :3], w[cam, 3:]
    loss_fn = MC_NeRF_Loss(sp)
    l_intr = loss_fn.get_reproject_loss([pd, h["pt_gt"]])
    total = l_intr / (l_intr.detach() + 1e-8) + ((g * rc + b - h["gt"]) ** 2).mean() + ((g * rf + b - h["gt"]) ** 2).mean() + REG * (w[cam] ** 2).mean()
    total.backward()
    assert abs(float(out[0]) - float(total.detach())) <= 2e-6 * max(1.0, abs(float(total.detach())))
    for got, want in ((d_pd, pd.grad), (d_c, rc.grad), (d_f, rf.grad)):
        assert float((got.cpu() - want).abs().max()) <= 2e-6 * float(want.abs().max()) + 1e-12
    # (an fp32 eager sum over the rays has its own rounding: the row is held to the fp64 restatement's bar, twice for the two sums)
    ref = R.grads(h["pd"], h["pt_gt"], H, W, True, h["rgb_c"], h["rgb_f"], h["gt"], h["color_w"], [cam], [0, n], REG)
    assert bool(((d_w.cpu().double() - ref["d_color"]).abs() <= 2e-6 * ref["abs_sum"]["d_color"] + 1e-12).all())
    assert bool(((d_w.cpu() - w.grad).abs().double() <= 4e-6 * ref["abs_sum"]["d_color"] + 1e-12).all())
    assert float(d_w[[i for i in range(c["C"]) if i != cam]].abs().max()) == 0.0
    # ... and through the loss module on device tensors
    via = loss_fn({"intr": [d["pd"], d["pt_gt"]], "rgb": [d["rgb_c"], d["rgb_f"], d["gt"]], "color": [d["color_w"], [cam], [0, n]]}, "GLOBAL_OPTIM_EPOCH")
    assert torch.equal(via, out[0])
    alone = loss_fn.get_rgb_loss_calibrated([d["rgb_c"], d["rgb_f"], d["gt"]], d["color_w"], [cam], [0, n])
    assert abs(float(alone) - (float(out[2]) + float(out[3]))) <= 2e-6


# ------------------------------------------------------------------------------------------------------------------ 5. the model
STAGE = "GLOBAL_OPTIM_EPOCH"
BATCH = 301
STEP_CAMS = [5, 0, 5]


def _step_setup(dev, K, **extra):
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model
    if K > 1:
        extra["cams_per_step"] = K
    sp = S.make_sys_param(dev, samples=32, scale=2, batch=BATCH, H=H, W=W, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision="f16x3", **extra)
    torch.manual_seed(3)
    model = MC_Model(sp).to(dev)
    S.init_cameras_near_gt(model)
    u8 = torch.randint(0, 256, (model.train_numb, H * W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    data = (DeviceImageSet(u8.to(dev), H, W), torch.tensor(STEP_CAMS[:K]), wpts, pts, wpts, pts)
    return sp, model, data


@pytest.mark.parametrize("K", [1, 3])
def test_model_step_carries_the_colour_key_and_trains_the_parameter(gpu_device, K):
    from mc_nerf_amd import ops
    from mc_nerf_amd.model import MC_NeRF_Loss, RAdam
    sp, model, data = _step_setup(gpu_device, K, color_calib="affine")
    assert len(model.state_dict()) == 47
    with torch.no_grad():
        model.weights_color.copy_(0.6 * torch.rand(model.train_numb, 6, generator=torch.Generator().manual_seed(8)) - 0.3)
    before = model.weights_color.detach().clone()
    loss_fn = MC_NeRF_Loss(sp)
    opt = RAdam(model.parameters(), lr=5e-4, weight_decay=0.0)
    torch.manual_seed(7)
    loss_dict, *_ = model(data, 20, STAGE, 0.5)
    assert set(loss_dict) == {"intr", "rgb", "color"}
    w, cams, seg = loss_dict["color"]
    # (the single-camera step draws without replacement from the camera's H W = 240 pixels: 240 rays of the batch of 301)
    assert w is model.weights_color and list(cams) == STEP_CAMS[:K] and list(seg) == (ops.ray_segments(BATCH, K) if K > 1 else [0, H * W])
    loss = loss_fn(loss_dict, STAGE)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    grad = model.weights_color.grad.detach().clone()
    assert bool(torch.isfinite(grad).all())
    outside = [c for c in range(model.train_numb) if c not in cams]
    assert float(grad[outside].abs().max()) == 0.0 and all(float(grad[c].abs().min()) > 0 for c in cams)
    cpu = lambda t: t.detach().cpu()
    (pd, pt_gt), (rgb_c, rgb_f, gt) = loss_dict["intr"], loss_dict["rgb"]
    ref = R.grads(cpu(pd), cpu(pt_gt), H, W, True, cpu(rgb_c), cpu(rgb_f), cpu(gt), cpu(before), cams, seg, 1e-3)
    assert abs(float(loss) - float(ref["value"])) <= 2e-6 * max(1.0, abs(float(ref["value"])))
    err = (grad.cpu().double() - ref["d_color"]).abs()
    print(f"[color calib, model step K={K}] d_color worst |err| / abs_sum {float((err / (ref['abs_sum']['d_color'] + 1e-300)).max()):.3e}")
    assert bool((err <= 2e-6 * ref["abs_sum"]["d_color"] + 1e-12).all())
    opt.step()
    assert opt.skipped_steps() == 0
    moved = (model.weights_color.detach() - before).abs()
    assert all(float(moved[c].min()) > 0 for c in cams) and bool(torch.isfinite(model.weights_color).all())


@pytest.mark.parametrize("K", [1, 3])
def test_model_without_the_key_emits_the_plain_loss_dict(gpu_device, K):
    from mc_nerf_amd.model import MC_NeRF_Loss
    sp, model, data = _step_setup(gpu_device, K)
    assert len(model.state_dict()) == 46 and not hasattr(model, "weights_color")
    torch.manual_seed(7)
    loss_dict, *_ = model(data, 20, STAGE, 0.5)
    assert set(loss_dict) == {"intr", "rgb"}
    assert bool(torch.isfinite(MC_NeRF_Loss(sp)(loss_dict, STAGE)))


# ------------------------------------------------------------------------------------------------------------------ 6. rendering
def test_render_as_a_camera_applies_its_correction(gpu_device):
    sp, model, data = _step_setup(gpu_device, 1, color_calib="affine")
    _, plain_model, _ = _step_setup(gpu_device, 1)                    # the same seed: the same nets
    with torch.no_grad():
        model.weights_color.copy_(0.6 * torch.rand(model.train_numb, 6, generator=torch.Generator().manual_seed(8)) - 0.3)
    torch.manual_seed(11)
    rgb, depth, opacity = model.render_image_device(2)
    torch.manual_seed(11)
    rgb0, depth0, opacity0 = plain_model.render_image_device(2)
    assert torch.equal(rgb, rgb0) and torch.equal(depth, depth0) and torch.equal(opacity, opacity0)      # the canonical scene: today's render
    torch.manual_seed(11)
    rgb4, depth4, _ = model.render_image_device(2, as_camera=4)
    gain, bias = model.color_correction()
    assert float((rgb4 - (gain[4] * rgb + bias[4])).abs().max()) <= 1e-6 and torch.equal(depth4, depth)
    assert float((rgb4 - rgb).abs().max()) > 1e-3
    with pytest.raises(ValueError, match="as_camera"):
        model.render_image_device(2, as_camera=model.train_numb)
    with pytest.raises(ValueError, match="color_calib"):
        plain_model.render_image_device(2, as_camera=0)


# ------------------------------------------------------------------------------------------------------------------ 7. convergence
def test_calibration_recovers_the_cameras_colour_responses(gpu_device):
    """500 steps of the radiance-field loop of tests/test_y_convergence_gpu._field_run (imported and run as it is by
    scripts/train_color_calib.field_run_with) in f16x3h from one seed on the procedural scene, float images: A clean images, no
    calibration; B the training images through camera_color_response(gain spread 0.15, bias spread 0.03), no calibration; C the images
    of B with the loss through get_rgb_loss_calibrated on a [C,6] parameter of its own in the loop's optimiser (a second group: lr 1e-2,
    no momentum -- the parameter is row-sparse in a one-camera loop; scripts/train_color_calib.py gives the reasoning).  Held-out PSNR
    against the CLEAN images, canonical render.  Conditions: C > B; C >= A - 3 dB (the margin of the voxel and pdf convergence tests);
    the recovered relative gains g / mean(g) of the training cameras closer (rms) to the true ones than identity is (ratio < 1).

    MEASURED (three runs of the script, profiles/color_calib_convergence.txt): A 22.77 / 23.02 / 22.80 dB, B 19.07 / 19.10 / 19.11 dB,
    C 21.69 / 21.26 / 21.52 dB, ratio 0.662 each time: C clears A - 3 dB by 1.2 dB or more.  On the DEFAULT path -- the colour parameter
    in the loop's one group, lr 2e-3, momentum 0.9 -- the rows moved a tenth of the way (C 19.65 - 19.81 dB, ratio 0.897, four runs) and
    C >= A - 3 dB failed in three of the four; with momentum at lr 1e-2 / 3e-2 / 1e-1: 19.5 / 20.0 - 20.7 / 8.2 dB.  The momentum-free
    group was chosen after those runs, on this scene.  At 2000 steps (default path): A 35.98, B 28.65, C 32.09 dB, ratio 0.537.  This
    test prints its line; the script writes the record.  (The ratio is not below 0.5: its assertion stays at < 1.)"""
    from scripts import train_color_calib as T
    r = T.experiment(gpu_device, steps=500)
    print("[color calib convergence] " + r["text"])          # (printed only: scripts/train_color_calib.py writes the record)
    assert all(math.isfinite(r[k]) for k in ("psnr_a", "psnr_b", "psnr_c", "gain_ratio"))
    assert r["psnr_c"] > r["psnr_b"]
    assert r["gain_ratio"] < 1.0
    assert r["psnr_c"] >= r["psnr_a"] - 3.0
