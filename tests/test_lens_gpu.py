"""The ray preamble with per-camera radial lens distortion (`lens_model` = "radial"; csrc/lens.hip) on the GPU.

At lens = 0 the fused forward is held to BIT identity with mcnerf_ray_batch_fwd; with a lens, forward and backward are gated against
the fp64 restatement tests/lens_ref.py relative to the pinhole kernels' own error plus a margin measured on the CPU with the
restatement's fp32 mode (tests/test_lens_cpu.py re-measures it on every run).  Inputs: lens_ref.CASES / make_case --
  a3  H, W = 37, 53, C = 4, cams [2, 0, 2], 1000 rays: 334 / 333 / 333, block 1 straddles segments, one camera twice, out of order;
  a1  the same camera set, K = 1 (the one-segment table of the single-camera step), 1000 rays: four blocks;
  b3  H, W = 20, 30, C = 3, cams [2, 0, 2], 5 rays: 2 / 2 / 1;   b3one  1 ray: segments 1 / 0 / 0 (empty segments);   b1  K = 1, 5 rays.
Every case has r_d <= 1.0, |k1| <= 0.08, |k2| <= 0.01; the tests assert min f' >= 0.5 over their own rays with the restatement."""
import os

import pytest
import torch

import lens_ref as R
import multicam_ref as MR
from mc_nerf_amd import synthetic as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
# 4 x the worst deviation of lens_ref's fp32 mode (the kernel's eight steps on the CPU) from its fp64 mode over all CASES, in units
# of 2^-24 (lens_ref.measure_margins; CPU-measured, recorded in profiles/lens_parity.txt):
M_F = 8.3           # forward: worst 2.07 units of max |rays_d| (case a3)
M_B = 146.0         # backward: worst magnitude-weighted per-ray relative error of the terms 36.40 units (d_kinv of case b3one: one ray)
ROBUST_ROWS = [[-5.0, 0.0], [50.0, 50.0], [0.5, -0.2], [-50.0, 50.0]]


@pytest.fixture(scope="module")
def scenes(gpu_device):
    """Per case: the host inputs of lens_ref.make_case and their device copies -- made once, shared, never written to."""
    out = {}
    for name in R.CASES:
        h = R.make_case(name)
        d = {k: (v.to(gpu_device) if isinstance(v, torch.Tensor) else v) for k, v in h.items()}
        d["zero"] = torch.zeros_like(d["lens"])
        out[name] = (h, d)
    return out


@pytest.fixture(scope="module")
def refs(scenes):
    """The fp64 references of every case, computed once: rays with and without the lens, gradients with and without the lens."""
    out = {}
    for name, (h, _) in scenes.items():
        a = (h["cams"], h["seg"], h["pix"], h["W"])
        d, o, fp, rd = R.rays(h["pose"], h["kinv"], h["lens"], *a)
        d0, o0 = MR.rays(h["pose"], h["kinv"], *a)
        out[name] = dict(d=d, o=o, fprime=fp, rd=rd, d0=d0, o0=o0, bwd=R.backward(h["pose"], h["kinv"], h["lens"], *a, h["g_d"], h["g_o"]),
                         bwd0=MR.backward(h["pose"], h["kinv"], *a, h["g_d"], h["g_o"]))
        assert float(fp.min()) >= 0.5 and float(rd.max()) <= 1.0, name          # the condition of every gate below
    return out


def _record(key, line):
    """profiles/lens_parity.txt: one line per key, rewritten by every run."""
    path = os.path.join(ROOT, "profiles", "lens_parity.txt")
    head = ("# lens_ray_batch_fwd / _bwd (csrc/lens.hip) against the fp64 restatement tests/lens_ref.py, beside ray_batch_fwd / _bwd at k = 0\n"
            "# against tests/multicam_ref.py (e_old); max abs error per tensor; margins in units of 2^-24: M_F = 8.3 = 4 x 2.07 (fp32 mode vs\n"
            "# fp64 mode, rays_d, worst case a3), M_B = 146 = 4 x 36.40 (per-ray terms, worst d_kinv of case b3one); CPU-measured by\n"
            "# lens_ref.measure_margins.  Written by tests/test_lens_gpu.py\n")
    try:
        lines = {}
        if os.path.isfile(path):
            lines = {l.split(":")[0]: l for l in open(path).read().splitlines() if l and not l.startswith("#")}
        lines[key] = f"{key}: {line}"
        with open(path, "w") as f:
            f.write(head + "\n".join(lines[k] for k in sorted(lines)) + "\n")
    except OSError:                     # (a read-only checkout: the figures are still printed)
        pass


# ------------------------------------------------------------------------------------------------------------------ 1 identity
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_zero_lens_is_the_pinhole_kernel_bit_for_bit(scenes, gpu_device, case):
    from mc_nerf_amd import ops
    _, s = scenes[case]
    a = (s["cams"], s["seg"], s["H"], s["W"])
    new = ops.lens_ray_batch_fwd(s["pose"], s["kinv"], s["zero"], *a, images=s["images"], pix=s["pix"])
    old = ops.ray_batch_fwd(s["pose"], s["kinv"], *a, images=s["images"], pix=s["pix"])
    assert new[0].dtype == torch.int64 and new[1].shape == (s["n"], 3)
    for x, y, name in zip(new, old, ("pix", "rays_d", "rays_o", "gt")):
        assert torch.equal(x, y), (case, name, "injected")
    assert ops.lens_ray_batch_fwd(s["pose"], s["kinv"], s["zero"], *a, pix=s["pix"])[3] is None
    for seed in (12345, 0x7FFFFFF0):                       # (the second one wraps past 2^32 from segment 1 on)
        word = torch.tensor([seed], dtype=torch.int32, device=gpu_device)
        new = ops.lens_ray_batch_fwd(s["pose"], s["kinv"], s["zero"], *a, images=s["images"], seed=word)
        old = ops.ray_batch_fwd(s["pose"], s["kinv"], *a, images=s["images"], seed=word)
        for x, y, name in zip(new, old, ("pix", "rays_d", "rays_o", "gt")):
            assert torch.equal(x, y), (case, name, "drawn", seed)
        bent = ops.lens_ray_batch_fwd(s["pose"], s["kinv"], s["lens"], *a, images=s["images"], seed=word)
        assert torch.equal(bent[0], old[0]) and torch.equal(bent[3], old[3]) and torch.equal(bent[2], old[2])
        assert not torch.equal(bent[1], old[1])


def test_torch_seed_governs_the_device_draw(scenes):
    from mc_nerf_amd import ops
    _, s = scenes["a3"]
    torch.manual_seed(11)
    p1 = ops.lens_ray_batch_fwd(s["pose"], s["kinv"], s["lens"], s["cams"], s["seg"], s["H"], s["W"])[0]
    torch.manual_seed(11)
    p2 = ops.ray_batch_fwd(s["pose"], s["kinv"], s["cams"], s["seg"], s["H"], s["W"])[0]
    assert torch.equal(p1, p2)


# ------------------------------------------------------------------------------------------------------------------ 2 forward
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_forward_against_fp64(scenes, refs, case):
    """Per output: e_new <= 2 e_old + M_F * 2^-24 * max|ref|, e_old the pinhole kernel's own error on the same pixels at k = 0."""
    from mc_nerf_amd import ops
    _, s = scenes[case]
    r = refs[case]
    a = (s["cams"], s["seg"], s["H"], s["W"])
    _, d, o, gt = ops.lens_ray_batch_fwd(s["pose"], s["kinv"], s["lens"], *a, images=s["images"], pix=s["pix"])
    _, d0, o0, gt0 = ops.ray_batch_fwd(s["pose"], s["kinv"], *a, images=s["images"], pix=s["pix"])
    assert torch.equal(gt, gt0)
    rec = []
    for name, new, old, ref, ref0 in (("rays_d", d, d0, r["d"], r["d0"]), ("rays_o", o, o0, r["o"], r["o0"])):
        e_old = float((old.cpu().double() - ref0).abs().max())
        e_new = float((new.cpu().double() - ref).abs().max())
        bound = 2.0 * e_old + M_F * U * float(ref.abs().max())
        rec.append(f"{name} e_old {e_old:.3e} e_new {e_new:.3e} bound {bound:.3e}")
        print(f"[lens fwd, case {case}] {rec[-1]}")
        assert e_new <= bound, (case, rec[-1])
    assert float((d.double().norm(dim=-1) - 1.0).abs().max()) <= 4 * U
    assert float((r["d"] - r["d0"]).abs().max()) > 1e-4 * min(1, s["n"])          # (the lens does bend these rays)
    _record(f"fwd {case}", "; ".join(rec) + f"; min f' {float(r['fprime'].min()):.3f} max r_d {float(r['rd'].max()):.3f}")


# ------------------------------------------------------------------------------------------------------------------ 3 robustness
@pytest.mark.parametrize("case", ["a3", "a1", "b3"])
def test_any_finite_coefficients_give_finite_unit_rays(scenes, case):
    """Outside the monotone region only finiteness is the contract: no comparison with the restatement."""
    from mc_nerf_amd import ops
    _, s = scenes[case]
    lens = torch.tensor(ROBUST_ROWS[:s["C"]] if case != "b3" else ROBUST_ROWS[1:], dtype=torch.float32, device=s["pose"].device)
    a = (s["cams"], s["seg"])
    pix, d, o, gt = ops.lens_ray_batch_fwd(s["pose"], s["kinv"], lens, *a, s["H"], s["W"], images=s["images"], pix=s["pix"])
    for t in (d, o, gt):
        assert bool(torch.isfinite(t).all())
    assert float((d.double().norm(dim=-1) - 1.0).abs().max()) <= 4 * U
    for t in ops.lens_ray_batch_bwd(s["pose"], s["kinv"], lens, *a, s["W"], s["pix"], s["g_d"], s["g_o"]):
        assert bool(torch.isfinite(t).all())


# ------------------------------------------------------------------------------------------------------------------ 4 backward
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_backward_against_fp64(scenes, refs, case):
    """d_pose, d_kinv: e_new <= 2 e_old + M_B * 2^-24 * max|ref|, e_old the pinhole backward's own error at k = 0.
    d_lens, per entry: e <= (M_B + 16) * 2^-24 * abs_sum, abs_sum the summed magnitudes of the entry's per-ray terms (16: the
    summation floor of tests/test_multicam_gpu.py)."""
    from mc_nerf_amd import ops
    _, s = scenes[case]
    r = refs[case]
    a = (s["cams"], s["seg"], s["W"], s["pix"], s["g_d"], s["g_o"])
    new_p, new_k, new_l = ops.lens_ray_batch_bwd(s["pose"], s["kinv"], s["lens"], *a)
    old_p, old_k = ops.ray_batch_bwd(s["pose"], s["kinv"], *a)
    C = s["C"]
    assert new_p.shape == (C, 3, 4) and new_k.shape == (C, 3, 3) and new_l.shape == (C, 2)
    used = sorted({c for k, c in enumerate(s["cams"]) if s["seg"][k + 1] > s["seg"][k]})
    unused = [c for c in range(C) if c not in used]
    for t in (new_p, new_k, new_l):
        assert float(t[unused].abs().max()) == 0.0
    ref = r["bwd"]
    for c in used:                      # the gates cannot pass on zeros
        assert float(ref["d_pose"][c].abs().max()) > 0 and float(ref["d_kinv"][c].abs().max()) > 0 and float(ref["d_lens"][c].abs().min()) > 0
    rec = []
    for name, new, old, ref0 in (("d_pose", new_p, old_p, r["bwd0"][0]), ("d_kinv", new_k, old_k, r["bwd0"][1])):
        e_old = float((old.cpu().double() - ref0).abs().max())
        e_new = float((new.cpu().double() - ref[name]).abs().max())
        big = float(ref[name].abs().max())
        bound = 2.0 * e_old + M_B * U * big
        rec.append(f"{name} e_old {e_old:.3e} e_new {e_new:.3e} bound {bound:.3e} max|ref| {big:.3e}")
        print(f"[lens bwd, case {case}] {rec[-1]}")
        assert e_new <= bound, (case, rec[-1])
    e = (new_l.cpu().double() - ref["d_lens"]).abs()
    bound = (M_B + 16.0) * U * ref["abs_sum"]["d_lens"]
    worst = float((e[used] / ref["abs_sum"]["d_lens"][used]).max()) / U
    rec.append(f"d_lens worst e / abs_sum {worst:.2f} units of 2^-24 (bound {M_B + 16.0:.0f}) max|ref| {float(ref['d_lens'].abs().max()):.3e}")
    print(f"[lens bwd, case {case}] {rec[-1]}")
    assert bool((e <= bound).all()), (case, rec[-1])
    _record(f"bwd {case}", "; ".join(rec))


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_backward_at_zero_lens_is_the_pinhole_backward(scenes, case):
    from mc_nerf_amd import ops
    _, s = scenes[case]
    a = (s["cams"], s["seg"], s["W"], s["pix"], s["g_d"], s["g_o"])
    new_p, new_k, new_l = ops.lens_ray_batch_bwd(s["pose"], s["kinv"], s["zero"], *a)
    old_p, old_k = ops.ray_batch_bwd(s["pose"], s["kinv"], *a)
    assert float((new_p - old_p).abs().max()) <= 16 * U * float(old_p.abs().max())
    assert float((new_k - old_k).abs().max()) <= 16 * U * float(old_k.abs().max())
    assert bool(torch.isfinite(new_l).all()) and float(new_l.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ 5 autograd
def test_lens_ray_batch_fn_is_differentiable_in_pose_kinv_and_lens(scenes):
    from mc_nerf_amd import ops
    from mc_nerf_amd.model.render import RayBatchFn
    _, s = scenes["a3"]
    pose, kinv, lens = (s[k].clone().requires_grad_(True) for k in ("pose", "kinv", "lens"))
    pix, d, o, gt = RayBatchFn.apply(pose, kinv, s["cams"], s["seg"], s["H"], s["W"], s["images"], s["pix"], None, lens)
    assert d.requires_grad and o.requires_grad and not pix.requires_grad and not gt.requires_grad
    ((d * s["g_d"]).sum() + (o * s["g_o"]).sum()).backward()
    dp, dk, dl = ops.lens_ray_batch_bwd(s["pose"], s["kinv"], s["lens"], s["cams"], s["seg"], s["W"], s["pix"], s["g_d"], s["g_o"])
    tol = 16.0 * U                          # (float atomics: the order of a row's few block sums is not fixed)
    for got, want in ((pose.grad, dp), (kinv.grad, dk), (lens.grad, dl)):
        assert got.shape == want.shape and float((got - want).abs().max()) <= tol * float(want.abs().max())


# ------------------------------------------------------------------------------------------------------------------ 6 recovery
def test_lens_is_recovered_from_rays_without_a_field(scenes, gpu_device):
    """The fp64 rays of a distorted camera are the target; weights start at zero, pose and K stay at the truth; Adam on the mean
    squared direction error through RayBatchFn.  The same loop on the restatement in fp64 sets the bar: the GPU loop must end
    within twice its final error plus 1e-4."""
    from mc_nerf_amd.model.render import RayBatchFn
    h, s = scenes[R.RECOVERY_CASE]
    cam = h["cams"][0]
    target = R.rays(h["pose"], h["kinv"], h["lens"], h["cams"], h["seg"], h["pix"], h["W"])[0]
    cpu = R.recovery_loop(lambda l: R.rays(h["pose"], h["kinv"], l, h["cams"], h["seg"], h["pix"], h["W"])[0], target, h["C"])
    gpu = R.recovery_loop(lambda l: RayBatchFn.apply(s["pose"], s["kinv"], s["cams"], s["seg"], s["H"], s["W"], None, s["pix"], None, l)[1],
                          target.float().to(gpu_device), h["C"], dtype=torch.float32, device=gpu_device).cpu()
    k1 = float(h["lens"][cam, 0])
    e_cpu, e_gpu = abs(float(cpu[cam, 0]) - k1), abs(float(gpu[cam, 0]) - k1)
    line = (f"k1* {k1:+.4f}: fp64 loop on the restatement |k1 - k1*| {e_cpu:.3e}, GPU loop {e_gpu:.3e} "
            f"({R.RECOVERY_STEPS} Adam steps, lr {R.RECOVERY_LR}, {h['n']} rays); k2* {float(h['lens'][cam, 1]):+.4f}, GPU k2 {float(gpu[cam, 1]):+.5f}")
    print(f"[lens recovery] {line}")
    _record("recovery", line)
    assert e_cpu < 1e-3
    assert e_gpu <= 2.0 * e_cpu + 1e-4, line
    others = [c for c in range(h["C"]) if c != cam]
    assert float(gpu[others].abs().max()) == 0.0            # cameras outside the table never move


# ------------------------------------------------------------------------------------------------------------------ 7 the model step
STAGE = "GLOBAL_OPTIM_EPOCH"
STEP_H, STEP_W, STEP_BATCH, STEP_CAMS = 20, 30, 301, [5, 0, 5]


def _step_model(dev, K, lens_model, extras):
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss
    kw = dict(extras)
    if K > 1:
        kw["cams_per_step"] = K
    if lens_model is not None:
        kw["lens_model"] = lens_model
    sp = S.make_sys_param(dev, samples=32, scale=2, batch=STEP_BATCH, H=STEP_H, W=STEP_W, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision="f32", **kw)
    torch.manual_seed(3)
    model = MC_Model(sp).to(dev)
    S.init_cameras_near_gt(model)
    u8 = torch.randint(0, 256, (model.train_numb, STEP_H * STEP_W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    data = (DeviceImageSet(u8.to(dev), STEP_H, STEP_W), torch.tensor(STEP_CAMS[:K]), wpts, pts, wpts, pts)
    return sp, model, data, MC_NeRF_Loss(sp)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("extras", [{}, {"color_calib": "affine", "pixel_sampler": "error"}], ids=["plain", "calib+error"])
def test_model_step_with_the_lens(gpu_device, K, extras):
    """Two NeRF-stage steps of a "radial" model with weights_lens left at zero beside the same steps of a "pinhole" model built from
    the same seed, the pixel draw injected through the existing hooks and torch's generator re-seeded per step: loss and rays_d are
    bit-equal.  Then the gradient: finite, non-zero on the step's cameras, exactly zero elsewhere.  (The reprojection term reaches
    every camera's row of weights_lens by design; for the row pattern it is given its own prediction as the observation, so that its
    residual and therefore its gradients are exactly zero and what arrives is the ray path's.)"""
    from mc_nerf_amd import ops
    dev = gpu_device
    seg = ops.ray_segments(STEP_BATCH, K)
    g = torch.Generator().manual_seed(21)
    draws = [torch.cat([torch.randperm(STEP_H * STEP_W, generator=g)[:b - a] for a, b in zip(seg, seg[1:])]).to(dev) for _ in range(2)]
    uniforms = [torch.rand(STEP_BATCH, 2, generator=g).to(dev) for _ in range(2)]
    results = {}
    for lens_model in ("radial", None):
        sp, model, data, loss_fn = _step_model(dev, K, lens_model, extras)
        seen, step = [], [0]
        model.nerf.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
        model.sample_pixels = lambda npix: draws[step[0]]
        model.sample_pixels_multi = lambda npix, seg_start: draws[step[0]]
        model.draw_error_uniforms = lambda n: uniforms[step[0]]
        losses = []
        for i in range(2):
            step[0] = i
            torch.manual_seed(100 + i)
            for p in model.parameters():
                p.grad = None
            loss_dict, *_ = model(data, 20, STAGE, 0.5)
            loss = loss_fn(loss_dict, STAGE)
            assert bool(torch.isfinite(loss))
            losses.append(loss.detach().clone())
            if lens_model == "radial":
                quiet = dict(loss_dict, intr=[loss_dict["intr"][0], loss_dict["intr"][0].detach()])
                loss_fn(quiet, STAGE).backward()
                gl = model.weights_lens.grad
                used = sorted(set(STEP_CAMS[:K]))
                others = [c for c in range(model.train_numb) if c not in used]
                assert gl is not None and bool(torch.isfinite(gl).all())
                assert all(float(gl[c].abs().min()) > 0 for c in used), gl[used]
                assert float(gl[others].abs().max()) == 0.0
                assert float(model.weights_pose.grad[used].abs().max()) > 0
        results[lens_model] = (losses, seen)
        if lens_model == "radial":
            assert model.lens_model == "radial" and torch.equal(model.lens_coefficients(), torch.zeros(model.train_numb, 2, device=dev))
    (l_new, d_new), (l_old, d_old) = results["radial"], results[None]
    assert len(d_new) == len(d_old) == 2
    for i in range(2):
        assert torch.equal(d_new[i], d_old[i]), i
        assert torch.equal(l_new[i], l_old[i]), (i, float(l_new[i]), float(l_old[i]))


def test_train_camera_rays_and_a_loaded_calibration(gpu_device):
    """A known calibration loaded into the parameter: train_camera_rays gives all H W rays of a training camera through its learnt
    pose, K and lens -- the restatement's rays for the same matrices."""
    sp, model, data, _ = _step_model(gpu_device, 1, "radial", {})
    lens = S.lens_distortion(model.train_numb, seed=2, k1_spread=0.04, k2_spread=0.005)
    with torch.no_grad():
        model.weights_lens.copy_(lens.to(gpu_device))
    d, o = model.train_camera_rays(7)
    assert d.shape == o.shape == (STEP_H * STEP_W, 3) and not d.requires_grad
    intr, pose, _ = model.add_weights2param(True, True, False)
    want_d, want_o, fp, _ = R.rays(pose.detach().cpu(), model.intr_inv_adj.detach().cpu(), model.lens_coefficients().cpu(), [7], [0, STEP_H * STEP_W],
                                   torch.arange(STEP_H * STEP_W), STEP_W)
    assert float(fp.min()) >= 0.5
    assert float((d.cpu().double() - want_d).abs().max()) <= 2e-6 and float((o.cpu().double() - want_o).abs().max()) <= 2e-6 * float(want_o.abs().max())
    with pytest.raises(ValueError, match="cam"):
        model.train_camera_rays(model.train_numb)


def test_default_step_launches_nothing_new(gpu_device, monkeypatch):
    """`lens_model` absent: the step never reaches the lens ops."""
    from mc_nerf_amd import ops
    from mc_nerf_amd.model import mc_nerf as M

    def no(*a, **kw):
        pytest.fail("a lens op ran in a pinhole step")
    monkeypatch.setattr(ops, "lens_ray_batch_fwd", no)
    monkeypatch.setattr(ops, "lens_ray_batch_bwd", no)
    monkeypatch.setattr(M, "distort_pixels", no)
    for K in (1, 3):
        sp, model, data, loss_fn = _step_model(gpu_device, K, None, {})
        loss_dict, *_ = model(data, 20, STAGE, 0.5)
        loss_fn(loss_dict, STAGE).backward()
        assert model.lens_model == "pinhole" and not hasattr(model, "weights_lens")
