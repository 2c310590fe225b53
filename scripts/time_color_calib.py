"""Times the colour-calibrated train loss (`color_calib` = "affine") against the plain one.

    python scripts/time_color_calib.py [out.txt] [--rays N] [--img S] [--steps N] [--windows N]        (needs the GPU)

Two measurements, both with device events and nothing but the measured work between them:
  * the loss launch alone at N = `rays`: mcnerf_train_loss (train_loss_kernel, unchanged by the feature) against
    mcnerf_train_loss_calib at K = 1 / 8 / 64, each entry point called on preallocated buffers, alternating inside every round;
  * the full single-camera train step (forward, loss, backward, RAdam) at the bench shape (Ball rig, 110 cameras, 32768 rays,
    64 x 2 samples, f16x3h, random-init selection) with the feature off and on, alternating windows, one model each from one seed.
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
        sys.exit("time_color_calib.py measures on the GPU; there is none here")
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    rays, img = opt_arg("--rays", 32768, int), opt_arg("--img", 800, int)
    steps, windows, warm = opt_arg("--steps", 10, int), opt_arg("--windows", 3, int), opt_arg("--warmup", 8, int)
    dev = torch.device("cuda:0")
    H = W = img
    C = 110
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    pd, ptg, rgb_c, rgb_f, gt, cw = r(1, C, 5, 2), r(1, C, 5, 2), r(rays, 3), r(rays, 3), r(rays, 3), (0.6 * r(C, 6) - 0.3)
    d_pd, d_c, d_f, d_w = torch.empty_like(pd), torch.empty_like(rgb_c), torch.empty_like(rgb_f), torch.empty_like(cw)
    out0 = torch.zeros(ops.TRAIN_LOSS_OUT, device=dev)
    out1 = torch.zeros(ops.TRAIN_LOSS_CALIB_OUT + ops.TRAIN_LOSS_CALIB_WS, device=dev)
    st = ops._stream()
    np_ = pd.numel() // 2

    def plain(i):
        _lib.call("mcnerf_train_loss", pd, ptg, np_, H, W, 1, rgb_c, rgb_f, gt, rgb_c.numel(), out0, d_pd, d_c, d_f, st)

    def calib_of(K):
        cams, start, _, n = ops._seg_arrays([(7 * k) % C for k in range(K)], ops.ray_segments(rays, K))

        def f(i):
            _lib.call("mcnerf_train_loss_calib", pd, ptg, np_, H, W, 1, rgb_c, rgb_f, gt, n, cw, C, cams, start, K, 1e-3,
                      out1, d_pd, d_c, d_f, d_w, out1[ops.TRAIN_LOSS_CALIB_OUT:], st)
        return f

    fns = {"train_loss": plain, **{f"train_loss_calib K = {K:2d}": calib_of(K) for K in (1, 8, 64)}}
    for f in fns.values():
        timed(f, 50)
    us = {k: [] for k in fns}
    for w in range(windows):
        for k, f in fns.items():
            us[k].append(1e3 * timed(f, 200))
    lines = [f"colour-calibrated train loss, one MI355X: {rays} rays, coarse + fine render, {C} cameras x 5 calibration points;",
             f"the entry point on preallocated buffers, 200 back-to-back launches per window (device events), {windows} windows, alternating"]
    for k, v in us.items():
        lines.append(f"{k:24s}: " + "  ".join(f"{x:7.2f}" for x in v) + f"  us per launch   (min {min(v):.2f})")

    runs = {}
    images = wpts = pts = None
    for on in (False, True):
        torch.manual_seed(42)
        sp = S.make_sys_param(dev, samples=64, scale=2, batch=rays, H=H, W=W, barf_mask=False, precision="f16x3h",
                              **({"color_calib": "affine"} if on else {}))
        model = MC_Model(sp).to(dev)
        S.init_cameras_near_gt(model, noise=1e-3)
        if runs:                    # one workspace pool for both models: their steps never overlap, the keys are the same
            model.nerf.ws_pool = runs[False]["model"].nerf.ws_pool
        model.nerf.reserve_workspaces(rays)
        if images is None:
            images = DeviceImageSet.synthetic(model.train_numb, H, W, dev, channels=4, seed=7)
            wpts, pts = (v.to(dev) for v in S.calibration_points(sp["gt_pose"], sp["intr_mat"][0]))
        runs[on] = dict(model=model, loss=MC_NeRF_Loss(sp), opt=RAdam(model.parameters(), lr=5e-4, weight_decay=4e-4))
    order = torch.randperm(runs[False]["model"].train_numb * 64, generator=torch.Generator().manual_seed(1)) % runs[False]["model"].train_numb

    def step_of(on):
        q = runs[on]

        def step(i):
            loss_dict, *_ = q["model"]((images, order[i:i + 1], wpts, pts, wpts, pts), 20, "GLOBAL_OPTIM_EPOCH", 0.6)
            loss = q["loss"](loss_dict, "GLOBAL_OPTIM_EPOCH")
            q["opt"].zero_grad(set_to_none=True)
            loss.backward()
            q["opt"].step()
        return step

    steps_of = {on: step_of(on) for on in runs}
    for on in runs:
        timed(steps_of[on], warm)
    ms = {on: [] for on in runs}
    for w in range(windows):
        for on in runs:
            ms[on].append(timed(lambda i: steps_of[on](warm + w * steps + i), steps))
    lines.append(f"full train step, Ball rig {H}x{W}, {rays} rays, 64x2 samples, f16x3h, random-init selection; {windows} windows of {steps} steps, alternating:")
    for on in runs:
        v = ms[on]
        lines.append(f"step  color_calib {'affine' if on else 'none  '}: " + "  ".join(f"{x:7.3f}" for x in v) + f"  ms/step   (min {min(v):.3f}, max {max(v):.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
