"""The multi-camera train step (`cams_per_step`; csrc/rays.hip) on the GPU.

A batch is K segments of consecutive rays, segment k of camera cam_k.  The fused forward is held to BIT identity with the three
single-camera kernels it stands for (sample_perm, raygen_fwd, gather_gt: the same arithmetic in the same order); the backward sums
the same fp32 terms as raygen_bwd in another order and is gated against the fp64 restatement of tests/multicam_ref.py relative to
raygen_bwd's own error; the model step is compared with the same step composed from the single-camera pieces.

Shapes, the smallest at which each indexing rule can go wrong:
  a  H, W = 12, 20 (non-square: a u / v swap shows), C = 7, cams [5, 0, 5], 301 rays: an uneven split 101 / 100 / 100, block 0 straddles
     segments 0 and 1, one camera twice, cameras out of order;
  b  cams [3, 1, 6, 2], 4 rays: one ray per segment, four segments in one wave;
  c  H = W = 32, cams [2, 4], 1500 rays: 750 per segment, several blocks per segment in the backward, n_k <= H W with little room."""
import os

import pytest
import torch

import multicam_ref as R
from conftest import load_golden, t
from mc_nerf_amd import synthetic as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"a": (12, 20, [5, 0, 5], 301), "b": (12, 20, [3, 1, 6, 2], 4), "c": (32, 32, [2, 4], 1500)}
C = 7
GOLDEN_RATIO = 0x9E3779B9


@pytest.fixture(scope="module")
def scenes(gpu_device):
    """Per shape: 7 distinct cameras (pose [C,3,4], kinv [C,3,3]), uint8 images [C, H W, 4], injected pixels, upstream gradients --
    made once, shared, never written to."""
    from mc_nerf_amd import ops
    out = {}
    for name, (H, W, cams, batch) in SHAPES.items():
        g = torch.Generator().manual_seed({"a": 1, "b": 2, "c": 3}[name])
        pose, K, _ = S.ball_cameras(0, H=H, W=W)
        sel = torch.randperm(pose.shape[0], generator=g)[:C]
        pose = pose[sel].float().contiguous()
        kinv = torch.linalg.inv(K[sel].double()).float()
        kinv = (kinv * (1.0 + 0.05 * torch.randn(C, 3, 3, generator=g))).contiguous()          # every camera its own intrinsics
        seg = ops.ray_segments(batch, len(cams))
        out[name] = dict(H=H, W=W, cams=cams, batch=batch, seg=seg, pose=pose.to(gpu_device), kinv=kinv.to(gpu_device),
                         images=torch.randint(0, 256, (C, H * W, 4), dtype=torch.uint8, generator=g).to(gpu_device),
                         pix=torch.randint(0, H * W, (batch,), generator=g).to(gpu_device),
                         g_d=torch.randn(batch, 3, generator=g).to(gpu_device), g_o=torch.randn(batch, 3, generator=g).to(gpu_device))
    return out


def _segments(s):
    return [(k, c, s["seg"][k], s["seg"][k + 1]) for k, c in enumerate(s["cams"])]


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape, channels", [("a", 4), ("b", 4), ("c", 4), ("a", 3)])
def test_forward_with_injected_pixels_is_the_single_camera_kernels_bit_for_bit(scenes, shape, channels):
    from mc_nerf_amd import ops
    s = scenes[shape]
    images = s["images"][..., :channels].contiguous()
    pix, d, o, gt = ops.ray_batch_fwd(s["pose"], s["kinv"], s["cams"], s["seg"], s["H"], s["W"], images=images, pix=s["pix"])
    assert pix.dtype == torch.int64 and torch.equal(pix, s["pix"])
    assert d.shape == o.shape == gt.shape == (s["batch"], 3)
    for k, c, lo, hi in _segments(s):
        pk = s["pix"][lo:hi].contiguous()
        d1, o1 = ops.raygen_fwd(s["pose"][c].contiguous(), s["kinv"][c].contiguous(), pk, s["W"])
        assert torch.equal(d[lo:hi], d1) and torch.equal(o[lo:hi], o1), (shape, k)
        assert torch.equal(gt[lo:hi], ops.gather_gt(images[c], pk)), (shape, k)
    # and without images there is no ground truth
    assert ops.ray_batch_fwd(s["pose"], s["kinv"], s["cams"], s["seg"], s["H"], s["W"], pix=s["pix"])[3] is None
    d64, o64 = R.rays(s["pose"].cpu(), s["kinv"].cpu(), s["cams"], s["seg"], s["pix"].cpu(), s["W"])
    assert float((d.cpu().double() - d64).abs().max()) < 2e-6 and float((o.cpu().double() - o64).abs().max()) < 2e-6 * float(o64.abs().max())


def _i32_word(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


@pytest.mark.parametrize("shape", ["a", "b", "c"])
@pytest.mark.parametrize("seed", [12345, 0x7FFFFFF0])          # (the second one wraps past 2^32 from segment 1 on)
def test_forward_device_draw_is_sample_perm_with_the_segment_key(scenes, gpu_device, shape, seed):
    from mc_nerf_amd import ops
    s = scenes[shape]
    npix = s["H"] * s["W"]
    word = torch.tensor([seed], dtype=torch.int32, device=gpu_device)
    pix, d, o, gt = ops.ray_batch_fwd(s["pose"], s["kinv"], s["cams"], s["seg"], s["H"], s["W"], images=s["images"], seed=word)
    drawn = []
    for k, c, lo, hi in _segments(s):
        key = torch.tensor([_i32_word(seed + k * GOLDEN_RATIO)], dtype=torch.int32, device=gpu_device)
        pk = pix[lo:hi]
        assert torch.equal(pk, ops.sample_perm(npix, hi - lo, gpu_device, seed=key)), (shape, k)
        assert int(pk.min()) >= 0 and int(pk.max()) < npix and pk.unique().numel() == hi - lo
        d1, o1 = ops.raygen_fwd(s["pose"][c].contiguous(), s["kinv"][c].contiguous(), pk.contiguous(), s["W"])
        assert torch.equal(d[lo:hi], d1) and torch.equal(o[lo:hi], o1)
        assert torch.equal(gt[lo:hi], ops.gather_gt(s["images"][c], pk.contiguous()))
        drawn.append(pk)
    if shape == "a":                    # the two segments of camera 5 (100 rays each) draw independently
        assert not torch.equal(drawn[0][:100], drawn[2])


def test_torch_seed_governs_the_device_draw(scenes, gpu_device):
    from mc_nerf_amd import ops
    s = scenes["a"]
    draw = lambda: ops.ray_batch_fwd(s["pose"], s["kinv"], s["cams"], s["seg"], s["H"], s["W"])[0]
    torch.manual_seed(11)
    p1 = draw()
    torch.manual_seed(11)
    p2 = draw()
    torch.manual_seed(11)
    first = ops.sample_perm(s["H"] * s["W"], s["seg"][1], gpu_device)         # segment 0 is the single-camera draw of the same word
    torch.manual_seed(12)
    p3 = draw()
    assert torch.equal(p1, p2) and torch.equal(p1[:s["seg"][1]], first) and not torch.equal(p1, p3)


# ------------------------------------------------------------------------------------------------------------------ backward
def _record_parity(shape, line):
    """profiles/multicam_parity.txt: one line per shape, rewritten by every run of the backward test."""
    path = os.path.join(ROOT, "profiles", "multicam_parity.txt")
    head = ("# ray_batch_bwd (csrc/rays.hip) against the fp64 restatement tests/multicam_ref.py, beside raygen_bwd summed over the same\n"
            "# segments (e_old); max abs error per tensor; written by tests/test_multicam_gpu.py::test_backward_against_fp64\n")
    try:
        lines = {}
        if os.path.isfile(path):
            lines = {l.split(":")[0]: l for l in open(path).read().splitlines() if l and not l.startswith("#")}
        lines[f"shape {shape}"] = f"shape {shape}: {line}"
        with open(path, "w") as f:
            f.write(head + "\n".join(lines[k] for k in sorted(lines)) + "\n")
    except OSError:                     # (a read-only checkout: the figures are still printed)
        pass


@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_backward_against_fp64(scenes, shape):
    """Gate per tensor: e_new <= 2 e_old + 16 * 2^-24 * max|ref| -- both kernels sum the same fp32 terms and differ only in their
    order (2 x), and the floor covers rows where the single-camera kernel happens to be exact."""
    from mc_nerf_amd import ops
    s = scenes[shape]
    pix = s["pix"]
    ref_p, ref_k = R.backward(s["pose"].cpu(), s["kinv"].cpu(), s["cams"], s["seg"], pix.cpu(), s["W"], s["g_d"].cpu(), s["g_o"].cpu())
    new_p, new_k = ops.ray_batch_bwd(s["pose"], s["kinv"], s["cams"], s["seg"], s["W"], pix, s["g_d"], s["g_o"])
    old_p, old_k = torch.zeros_like(new_p), torch.zeros_like(new_k)
    for k, c, lo, hi in _segments(s):
        dp, dk = ops.raygen_bwd(s["pose"][c].contiguous(), s["kinv"][c].contiguous(), pix[lo:hi].contiguous(), s["W"],
                                s["g_d"][lo:hi].contiguous(), s["g_o"][lo:hi].contiguous())
        old_p[c] += dp
        old_k[c] += dk
    assert new_p.shape == (C, 3, 4) and new_k.shape == (C, 3, 3)
    unused = [c for c in range(C) if c not in s["cams"]]
    assert float(new_p[unused].abs().max()) == 0.0 and float(new_k[unused].abs().max()) == 0.0
    assert all(float(ref_p[c].abs().max()) > 0 for c in s["cams"])
    rec = []
    for name, new, old, ref in (("d_pose", new_p, old_p, ref_p), ("d_kinv", new_k, old_k, ref_k)):
        e_old = float((old.cpu().double() - ref).abs().max())
        e_new = float((new.cpu().double() - ref).abs().max())
        big = float(ref.abs().max())
        bound = 2.0 * e_old + 16.0 * 2.0 ** -24 * big
        rec.append(f"{name} e_old {e_old:.3e} e_new {e_new:.3e} bound {bound:.3e} max|ref| {big:.3e}")
        print(f"[multicam bwd, shape {shape}] {rec[-1]}")
        assert e_new <= bound, (shape, rec[-1])
    _record_parity(shape, "; ".join(rec))


def test_ray_batch_fn_is_differentiable_in_pose_and_kinv(scenes):
    from mc_nerf_amd import ops
    from mc_nerf_amd.model.render import RayBatchFn
    s = scenes["a"]
    pose, kinv = s["pose"].clone().requires_grad_(True), s["kinv"].clone().requires_grad_(True)
    pix, d, o, gt = RayBatchFn.apply(pose, kinv, s["cams"], s["seg"], s["H"], s["W"], s["images"], s["pix"])
    assert d.requires_grad and o.requires_grad and not pix.requires_grad and not gt.requires_grad
    ((d * s["g_d"]).sum() + (o * s["g_o"]).sum()).backward()
    dp, dk = ops.ray_batch_bwd(s["pose"], s["kinv"], s["cams"], s["seg"], s["W"], s["pix"], s["g_d"], s["g_o"])
    tol = 16.0 * 2.0 ** -24                 # (float atomics: the order of a row's few block sums is not fixed)
    assert float((pose.grad - dp).abs().max()) <= tol * float(dp.abs().max())
    assert float((kinv.grad - dk).abs().max()) <= tol * float(dk.abs().max())


# ------------------------------------------------------------------------------------------------------------------ the model step
STAGE = "GLOBAL_OPTIM_EPOCH"
CAM_TENSORS = ["weights_pose", "weights_fx", "weights_fy", "weights_ux", "weights_uy", "weights_pose_intr"]


def _step_setup(dev, K=3, precision="f32", host_stack=False, seed=5):
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model
    H, W, cams, batch = SHAPES["a"]
    extra = {"cams_per_step": K} if K > 1 else {}
    sp = S.make_sys_param(dev, samples=32, scale=2, batch=batch, H=H, W=W, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision=precision, **extra)
    torch.manual_seed(3)
    model = MC_Model(sp).to(dev)
    S.init_cameras_near_gt(model)
    u8 = torch.randint(0, 256, (model.train_numb, H * W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    images = DeviceImageSet(u8.to(dev), H, W)
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    if host_stack:                  # what the reference's loader delivers, K items stacked: float images [K,H,W,3] (blended on white)
        f = u8[cams].float() / 255.0
        first = (f[..., :3] * f[..., 3:] + (1.0 - f[..., 3:])).reshape(K, H, W, 3)
    else:
        first = images
    data = (first, torch.tensor(cams[:K]), wpts, pts, wpts, pts)
    return sp, model, images, data


def test_model_step_matches_the_step_composed_from_single_camera_pieces(gpu_device):
    """`cams_per_step` = 3 in the joint stage, f32, pixels and the renderer's draws injected, against the same step put together from
    RaygenFn / gather_gt per segment on the same model.  Rays and gt handed on: bit-equal; loss: 1e-6 relative; camera gradients:
    1e-4 of each tensor's largest reference entry (the project's parity bar, per tensor); rows of cameras outside {0, 5}: exactly 0."""
    from mc_nerf_amd import ops
    from mc_nerf_amd.model import MC_NeRF_Loss
    from mc_nerf_amd.model.render import RaygenFn
    dev = gpu_device
    H, W, cams, batch = SHAPES["a"]
    sp, model, images, data = _step_setup(dev)
    seg = ops.ray_segments(batch, 3)
    g = torch.Generator().manual_seed(21)
    pix = torch.cat([torch.randperm(H * W, generator=g)[:b - a] for a, b in zip(seg, seg[1:])]).to(dev)
    draws = dict(jitter=(torch.rand(batch, 1, generator=g) * (sp["far"] - sp["near"]) / 32).to(dev), eps_c=torch.randn(batch, 32, generator=g).to(dev),
                 eps_sel=torch.randn(batch, 32, generator=g).to(dev), eps_f=torch.randn(batch, 64, generator=g).to(dev))
    model.sample_pixels_multi = lambda npix, seg_start: pix
    orig, seen = model.nerf.render_rays_train, []

    def replay(d, o, e, r, only_coarse=False):
        seen.append((d.detach().clone(), o.detach().clone()))
        return orig(d, o, e, r, only_coarse, **draws)
    model.nerf.render_rays_train = replay
    loss_fn = MC_NeRF_Loss(sp)

    def grads():
        out = {n: getattr(model, n).grad.detach().clone() for n in CAM_TENSORS}
        for p in model.parameters():
            p.grad = None
        return out

    # ---- the K-camera step
    loss_dict, _, _, rays_valid = model(data, 20, STAGE, 0.5)
    loss = loss_fn(loss_dict, STAGE)
    loss.backward()
    got, got_loss, got_gt = grads(), float(loss.detach()), loss_dict["rgb"][2].clone()
    assert model.opt_idx == 1 and model.last_step_segments == (cams, seg) and torch.equal(model.last_step_pix, pix)
    with torch.no_grad():
        dv, ov = model.get_rays(model.valid_pose, cams[0], model.intr_val_inv)         # the first id keeps today's role
    assert torch.equal(rays_valid[0], dv) and torch.equal(rays_valid[1], ov)

    # ---- the same step from the single-camera pieces
    wpts, pts = data[2].to(dev), data[3].to(dev)

    def composed():
        model.nerf.emmbedding_xyz.barf_mode = True
        intr_adj, pose_adj, calib = model.add_weights2param(True, True, True, wpts, None)
        reproj = model._reproject(wpts, intr_adj, calib, 0)
        kinv = model.intr_inv_adj
        ds, os_, gts = [], [], []
        for k, c in enumerate(cams):
            pk = pix[seg[k]:seg[k + 1]].contiguous()
            d, o = RaygenFn.apply(pose_adj[c], kinv[c], pk, W)
            ds.append(d), os_.append(o), gts.append(ops.gather_gt(images.images[c], pk))
        rgb_c, rgb_f = model.nerf(torch.cat(ds), torch.cat(os_), 20, 0.5)
        ld = {"intr": [reproj, pts], "rgb": [rgb_c, rgb_f, torch.cat(gts)]}
        l = loss_fn(ld, STAGE)
        l.backward()
        return grads(), float(l.detach()), ld["rgb"][2]
    ref, ref_loss, ref_gt = composed()
    ref2, _, _ = composed()
    assert len(seen) == 3
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])          # the rays handed to the renderer
    assert torch.equal(got_gt, ref_gt)
    assert abs(got_loss - ref_loss) <= 1e-6 * abs(ref_loss), (got_loss, ref_loss)
    gp = got["weights_pose"]
    others = [c for c in range(gp.shape[0]) if c not in (0, 5)]
    assert float(gp[others].abs().max()) == 0.0
    assert float(gp[0].abs().max()) > 0 and float(gp[5].abs().max()) > 0
    for n in CAM_TENSORS:
        big = float(ref[n].abs().max())
        e, spread = float((got[n] - ref[n]).abs().max()), float((ref2[n] - ref[n]).abs().max())
        print(f"[multicam step] {n}: |fused - composed| {e:.3e}, composed run-to-run {spread:.3e}, max|ref| {big:.3e}")
        assert big > 0 and e <= 1e-4 * big, (n, e, big)


# ------------------------------------------------------------------------------------------------------------------ defaults
def test_default_step_still_runs_the_single_camera_kernels(gpu_device, monkeypatch):
    """`cams_per_step` absent, the set-up of test_model_gpu.py::test_mc_model_step_with_the_device_side_pixel_draw: the step calls
    sample_pixels and RaygenFn (sample_perm, raygen_fwd, gather_gt) and never the fused kernel."""
    from mc_nerf_amd import ops
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model
    from mc_nerf_amd.model import mc_nerf as M
    g = load_golden("g11_mc_model_step")
    dev = gpu_device
    H, W, B, cam = int(g["H"]), int(g["W"]), int(g["B"]), int(g["cam"])
    sp = S.make_sys_param(dev, samples=32, scale=2, batch=B, H=H, W=W, coarse=(4, 32, [2]), fine=(8, 64, [4]),
                          barf_start=float(g["barf"][0]), barf_end=float(g["barf"][1]), precision="f16x3")
    model = MC_Model(sp).to(dev)
    model.load_state_dict({k[2:]: t(v) for k, v in g.items() if k.startswith("p.")})
    assert model.cams_per_step == 1
    u8 = torch.randint(0, 256, (model.train_numb, H * W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    calls = {}

    def count(mod, name, key):
        fn = getattr(mod, name)

        def wrapped(*a, **kw):
            calls[key] = calls.get(key, 0) + 1
            return fn(*a, **kw)
        monkeypatch.setattr(mod, name, wrapped)
    for name in ("sample_perm", "raygen_fwd", "gather_gt", "ray_batch_fwd"):
        count(ops, name, name)

    class NoRayBatch:
        @staticmethod
        def apply(*a, **kw):
            pytest.fail("RayBatchFn ran in a single-camera step")
    monkeypatch.setattr(M, "RayBatchFn", NoRayBatch)
    draw = model.sample_pixels

    def spy(npix):
        calls["sample_pixels"] = calls.get("sample_pixels", 0) + 1
        return draw(npix)
    model.sample_pixels = spy
    data = (DeviceImageSet(u8.to(dev), H, W), torch.tensor([cam]), t(g["wpts"]), t(g["pts"]), t(g["wpts_e"]), t(g["pts_e"]))
    loss_dict, *_ = model(data, 20, STAGE, float(g["cur_ratio"]))
    assert calls.get("sample_pixels") == 1 and calls.get("sample_perm") == 1 and calls.get("gather_gt") == 1
    assert calls.get("raygen_fwd") == 2 and "ray_batch_fwd" not in calls               # (train rays + the validation rays)
    assert model.last_step_segments is None and loss_dict["rgb"][2].shape == (B, 3)


def test_five_multicamera_steps_with_radam(gpu_device):
    from mc_nerf_amd.model import MC_NeRF_Loss, RAdam
    sp, model, images, data = _step_setup(gpu_device, precision="f16x3")
    loss_fn = MC_NeRF_Loss(sp)
    opt = RAdam(model.parameters(), lr=5e-4, weight_decay=0.0)
    torch.manual_seed(7)
    losses, pixels = [], []
    for step in range(5):
        loss_dict, *_ = model(data, 20, STAGE, 0.5)
        loss = loss_fn(loss_dict, STAGE)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        pixels.append(model.last_step_pix)
    assert bool(torch.isfinite(torch.stack(losses)).all()) and opt.skipped_steps() == 0
    assert not torch.equal(pixels[0], pixels[1])                   # every step draws its own pixels
    seg = model.last_step_segments[1]
    for a, b in zip(seg, seg[1:]):
        assert pixels[-1][a:b].unique().numel() == b - a


def test_host_float_stack_gives_the_resident_sets_ground_truth(gpu_device):
    """A host float stack [K,H,W,3] (the reference's loader with a batch of K): gt[i] = stack[segment of i, pix[i]], the same values
    the resident uint8 set gives for the same images."""
    from mc_nerf_amd import ops
    H, W, cams, batch = SHAPES["a"]
    seg = ops.ray_segments(batch, 3)
    pix = torch.cat([torch.randperm(H * W, generator=torch.Generator().manual_seed(9 + k))[:b - a] for k, (a, b) in enumerate(zip(seg, seg[1:]))])
    gts = []
    for host in (False, True):
        sp, model, images, data = _step_setup(gpu_device, host_stack=host)
        model.sample_pixels_multi = lambda npix, seg_start: pix.to(gpu_device)
        loss_dict, *_ = model(data, 20, STAGE, 0.5)
        gts.append(loss_dict["rgb"][2])
    u8 = images.images.cpu()            # (the restatement runs on the host: torch's device division by a scalar multiplies by 1 / 255)
    want = torch.cat([R.gt_from_u8(u8, c, pix[a:b]) for c, a, b in zip(cams, seg, seg[1:])])
    assert gts[0].shape == (batch, 3) and torch.equal(gts[0], gts[1]) and torch.equal(gts[0].cpu(), want)
