"""Times the ray preamble with per-camera radial lens distortion (`lens_model` = "radial").

    python scripts/time_lens.py [out.txt] [--rays N] [--img S] [--steps N] [--windows N]        (needs the GPU)

Two measurements, both with device events and nothing but the measured work between them:
  * the two new launches alone at N = `rays`, an `img` x `img` image, K = 1 / 8 / 64: mcnerf_lens_ray_batch_fwd / _bwd on preallocated
    buffers next to mcnerf_ray_batch_fwd / _bwd on the same table, pixels and upstream gradients, alternating inside every round, and
    the eager reprojection op (lens.distort_pixels, forward + backward on C x 5 points) the feature adds to every step;
  * the full train step (forward, loss, backward, RAdam) at the bench shape (Ball rig, 110 cameras, 32768 rays, 64 x 2 samples,
    f16x3h, random-init selection) with the feature off and on, alternating windows, one model each from one seed: the
    single-camera step and the 64-camera step.  With the feature on the step also runs the eager reprojection op (a dozen small torch
    launches each way on C x 5 points).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mc_nerf_amd import _lib, ops, synthetic as S  # noqa: E402
from mc_nerf_amd.data import DeviceImageSet  # noqa: E402
from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, RAdam  # noqa: E402


def opt_arg(name, default, cast):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    if not torch.cuda.is_available():
        sys.exit("time_lens.py measures on the GPU; there is none here")
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    rays, img = opt_arg("--rays", 32768, int), opt_arg("--img", 800, int)
    steps, windows, warm = opt_arg("--steps", 20, int), opt_arg("--windows", 3, int), opt_arg("--warmup", 8, int)
    dev = torch.device("cuda:0")
    H = W = img
    C = 110
    g = torch.Generator().manual_seed(0)
    pose, Kmat, _ = S.ball_cameras(0, H=H, W=W)
    pose, kinv = pose.to(dev).contiguous(), torch.linalg.inv(Kmat).to(dev).contiguous()
    lens = S.lens_distortion(C, seed=1).to(dev).contiguous()
    images = DeviceImageSet.synthetic(C, H, W, dev, channels=4, seed=7)
    pix = torch.randint(0, H * W, (rays,), generator=g).to(dev)
    g_d, g_o = torch.randn(rays, 3, generator=g).to(dev), torch.randn(rays, 3, generator=g).to(dev)
    pix_out = torch.empty(rays, dtype=torch.int64, device=dev)
    d, o, gt = (torch.empty(rays, 3, device=dev) for _ in range(3))
    grads = torch.zeros(C * 23, device=dev)
    d_pose, d_kinv, d_lens = grads[:C * 12], grads[C * 12:C * 21], grads[C * 21:]
    st = ops._stream()
    u8 = images.images

    def quad_of(K):
        cams, start, _, n = ops._seg_arrays([(7 * k) % C for k in range(K)], ops.ray_segments(rays, K))

        def fwd(i):
            _lib.call("mcnerf_ray_batch_fwd", pose, kinv, C, cams, start, K, n, H, W, pix, None, u8,
                      int(u8.shape[-1]), pix_out, d, o, gt, st)

        def bwd(i):
            _lib.call("mcnerf_ray_batch_bwd", pose, kinv, C, cams, start, K, n, W, pix, g_d, g_o, d_pose, d_kinv, st)

        def lfwd(i):
            _lib.call("mcnerf_lens_ray_batch_fwd", pose, kinv, lens, C, cams, start, K, n, H, W, pix, None,
                      u8, int(u8.shape[-1]), pix_out, d, o, gt, st)

        def lbwd(i):
            _lib.call("mcnerf_lens_ray_batch_bwd", pose, kinv, lens, C, cams, start, K, n, W, pix, g_d, g_o,
                      d_pose, d_kinv, d_lens, st)
        return fwd, lfwd, bwd, lbwd

    fns = {}
    for K in (1, 8, 64):
        for name, f in zip(("ray_batch_fwd", "lens_ray_batch_fwd", "ray_batch_bwd", "lens_ray_batch_bwd"), quad_of(K)):
            fns[f"{name} K = {K:2d}"] = f
    # the eager reprojection op of the feature, forward + backward, on the step's C x 5 tag pixels (a few dozen small torch launches)
    from mc_nerf_amd.lens import distort_pixels
    tag = (torch.rand(1, C, 5, 2, generator=g) * H).to(dev).requires_grad_(True)
    Kd, lens_p = Kmat.to(dev).requires_grad_(True), lens.clone().requires_grad_(True)

    def reproject(i):
        distort_pixels(tag, Kd, lens_p).sum().backward()
    fns["distort_pixels fwd + bwd"] = reproject
    for f in fns.values():
        timed(f, 50)
    us = {k: [] for k in fns}
    for w in range(windows):
        for k, f in fns.items():
            us[k].append(1e3 * timed(f, 200))
    lines = [f"ray preamble with radial lens distortion, one MI355X: {rays} rays, {C} cameras of {H}x{W}, injected pixels, 4-channel images;",
             f"each entry point on preallocated buffers (one launch; distort_pixels: eager torch, .sum().backward() included), 200 back-to-back calls per window (device events), {windows} windows, alternating"]
    for k, v in us.items():
        lines.append(f"{k:28s}: " + "  ".join(f"{x:7.2f}" for x in v) + f"  us per call   (min {min(v):.2f})")

    configs = {"K =  1  pinhole": (1, {}), "K =  1  radial": (1, {"lens_model": "radial"}),
               "K = 64  pinhole": (64, {}), "K = 64  radial": (64, {"lens_model": "radial"})}
    runs = {}
    wpts = pts = None
    for name, (K, extra) in configs.items():
        torch.manual_seed(42)
        sp = S.make_sys_param(dev, samples=64, scale=2, batch=rays, H=H, W=W, barf_mask=False, precision="f16x3h",
                              **({"cams_per_step": K} if K > 1 else {}), **extra)
        model = MC_Model(sp).to(dev)
        S.init_cameras_near_gt(model, noise=1e-3)
        if extra:                           # a non-zero lens, so that the iteration has something to do
            with torch.no_grad():
                model.weights_lens.copy_(lens)
        if runs:                            # one workspace pool for all models: their steps never overlap, the keys are the same
            model.nerf.ws_pool = next(iter(runs.values()))["model"].nerf.ws_pool
        model.nerf.reserve_workspaces(rays)
        if wpts is None:
            wpts, pts = (v.to(dev) for v in S.calibration_points(sp["gt_pose"], sp["intr_mat"][0]))
        runs[name] = dict(K=K, model=model, loss=MC_NeRF_Loss(sp), opt=RAdam(model.parameters(), lr=5e-4, weight_decay=4e-4))
    order = torch.randperm(C * 64, generator=torch.Generator().manual_seed(1)) % C      # the camera ids of the steps, host side

    def step_of(name):
        q = runs[name]
        K = q["K"]

        def step(i):
            cams = order[(i * K) % (order.numel() - K):][:K]
            loss_dict, *_ = q["model"]((images, cams, wpts, pts, wpts, pts), 20, "GLOBAL_OPTIM_EPOCH", 0.6)
            loss = q["loss"](loss_dict, "GLOBAL_OPTIM_EPOCH")
            q["opt"].zero_grad(set_to_none=True)
            loss.backward()
            q["opt"].step()
        return step

    steps_of = {name: step_of(name) for name in runs}
    for name in runs:
        timed(steps_of[name], warm)
    ms = {name: [] for name in runs}
    for w in range(windows):
        for name in runs:
            ms[name].append(timed(lambda i: steps_of[name](warm + w * steps + i), steps))
    lines.append(f"full train step, Ball rig {H}x{W}, {rays} rays, 64x2 samples, f16x3h, random-init selection; {windows} windows of {steps} steps each,")
    lines.append("alternating; K = cams_per_step:")
    for name, v in ms.items():
        lines.append(f"step  {name:16s}: " + "  ".join(f"{x:7.3f}" for x in v) + f"  ms/step   (min {min(v):.3f}, max {max(v):.3f})")
    for off, on in (("K =  1  pinhole", "K =  1  radial"), ("K = 64  pinhole", "K = 64  radial")):
        lo, hi, m = min(ms[off]), max(ms[off]), sum(ms[on]) / len(ms[on])
        where = "inside" if lo <= m <= hi else f"{m - hi:.3f} ms above" if m > hi else f"{lo - m:.3f} ms below"
        lines.append(f"  '{on}' mean {m:.3f} ms: {where} the window spread of '{off}' [{lo:.3f}, {hi:.3f}]")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
