"""Times depth supervision (`depth_weight`) against today's path.

    python scripts/time_depth.py [out.txt] [--rays N] [--img S] [--steps N] [--windows N]        (needs the GPU)

Two measurements, both with device events and nothing but the measured work between them:
  * the kernels alone at N = `rays`, S = 64 and 128 (semi-transparent rays): mcnerf_geo_depth_fwd beside mcnerf_ext_front_weight (the
    same fp64 sweep with another sum) and mcnerf_composite_fwd (the train call's form: with selection weights);
    mcnerf_geo_composite_bwd_z with d_zexp, and with all four gradients, beside mcnerf_reg_composite_bwd_w (with d_dist + d_fg) and
    mcnerf_composite_bwd; mcnerf_geo_gather_depth and mcnerf_geo_depth_loss (both launches) at N rays, half of the targets valid; each
    entry point on preallocated buffers, alternating inside every round;
  * the full single-camera train step (forward, loss, backward, RAdam) at the bench shape (Ball rig, 110 cameras, 32768 rays,
    64 x 2 samples, f16x3h, random-init selection) with the key off (today's path) and on, alternating windows of one process, one
    model each from one seed; the depth images are random targets in (near, far), half of them "no measurement".
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mc_nerf_amd import _ext, _geo, _lib, _reg, ops, synthetic as S  # noqa: E402
from mc_nerf_amd.data import DeviceImageSet  # noqa: E402
from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, RAdam  # noqa: E402

LAMBDA = 0.1


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


def kernel_lines(dev, rays, S_, windows):
    g = torch.Generator().manual_seed(S_)
    tau = 0.1 + 2.9 * torch.rand(rays, 1, generator=g)
    sig = torch.log(torch.expm1(tau / 7.0)) + 0.3 * torch.randn(rays, S_, generator=g)
    sr = torch.cat([sig.unsqueeze(-1), torch.rand(rays, S_, 3, generator=g)], -1).contiguous().to(dev)
    d = torch.nn.functional.normalize(torch.randn(rays, 3, generator=g), dim=-1).to(dev)
    z, jit = torch.linspace(1, 8, S_).to(dev), (torch.rand(rays, generator=g) * 7.0 / S_).to(dev)
    eps, eps_sel = (0.3 * torch.randn(rays, S_, generator=g)).to(dev), (0.3 * torch.randn(rays, S_, generator=g)).to(dev)
    d_rgb, d_fg, d_dist = torch.randn(rays, 3, generator=g).to(dev), torch.randn(rays, generator=g).to(dev), torch.randn(rays, generator=g).to(dev)
    d_zexp, zexp = torch.randn(rays, generator=g).to(dev), torch.empty(rays, device=dev)
    depth = 1.0 + 7.0 * torch.rand(4, 800 * 800, generator=g)
    depth[torch.rand(4, 800 * 800, generator=g) < 0.5] = 0.0
    depth, pix = depth.to(dev), torch.randint(0, 800 * 800, (rays,), generator=g).to(dev)
    import ctypes
    seg_cam, seg_start = (ctypes.c_int32 * 1)(2), (ctypes.c_int32 * 2)(0, rays)
    d_gt, zexp_f, d_c, d_f = torch.empty(rays, device=dev), (1.0 + 7.0 * torch.rand(rays, generator=g)).to(dev), torch.empty(rays, device=dev), torch.empty(rays, device=dev)
    loss_out = torch.zeros(ops.DEPTH_LOSS_OUT, device=dev)
    rgb, w_sel, wmax = torch.empty(rays, 3, device=dev), torch.empty(rays, S_, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    fg, dist, mom = torch.empty(rays, device=dev), torch.empty(rays, device=dev), torch.empty(rays, ops.DIST_MOMENT_BYTES, dtype=torch.uint8, device=dev)
    d_out, gmax = torch.empty(rays, S_, 4, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    st = ops._stream()
    zn, zs = 1.0, 1.0 / 7.0
    fns = {
        "composite_fwd": lambda i: _lib.call("mcnerf_composite_fwd", sr, d, z, 0, jit, eps, eps_sel, rays, S_, 1, rgb, None, None, w_sel, wmax, st),
        "ext_front_weight": lambda i: _ext.call("mcnerf_ext_front_weight", sr, z, 0, jit, eps, rays, S_, fg, st),
        "reg_distortion_fwd": lambda i: _reg.call("mcnerf_reg_distortion_fwd", sr, z, 0, jit, eps, rays, S_, zn, zs, dist, mom, st),
        "geo_depth_fwd": lambda i: _geo.call("mcnerf_geo_depth_fwd", sr, z, 0, jit, eps, rays, S_, zexp, st),
        "composite_bwd": lambda i: _lib.call("mcnerf_composite_bwd", sr, z, 0, jit, eps, d_rgb, rays, S_, 1, d_out, gmax, st),
        "reg_composite_bwd_w dist+fg": lambda i: _reg.call("mcnerf_reg_composite_bwd_w", sr, z, 0, jit, eps, d_rgb, d_fg, d_dist, mom, zn, zs, rays, S_, 1, d_out, gmax, st),
        "geo_composite_bwd_z zexp": lambda i: _geo.call("mcnerf_geo_composite_bwd_z", sr, z, 0, jit, eps, d_rgb, None, None, None, d_zexp, zn, zs, rays, S_, 1, d_out, gmax, st),
        "geo_composite_bwd_z all four": lambda i: _geo.call("mcnerf_geo_composite_bwd_z", sr, z, 0, jit, eps, d_rgb, d_fg, d_dist, mom, d_zexp, zn, zs, rays, S_, 1, d_out, gmax, st),
        "geo_gather_depth": lambda i: _geo.call("mcnerf_geo_gather_depth", depth, 4, 800 * 800, seg_cam, seg_start, 1, pix, rays, d_gt, st),
        "geo_depth_loss (2 launches)": lambda i: _geo.call("mcnerf_geo_depth_loss", zexp, zexp_f, d_gt, rays, zn, zs, 0.1, loss_out, d_c, d_f, st),
    }
    for f in fns.values():
        timed(f, 50)
    us = {k: [] for k in fns}
    for w in range(windows):
        for k, f in fns.items():
            us[k].append(1e3 * timed(f, 200))
    return [f"S = {S_:3d}  {k:30s}: " + "  ".join(f"{x:7.2f}" for x in v) + f"  us per launch   (min {min(v):.2f})" for k, v in us.items()]


def main():
    if not torch.cuda.is_available():
        sys.exit("time_depth.py measures on the GPU; there is none here")
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    rays, img = opt_arg("--rays", 32768, int), opt_arg("--img", 800, int)
    steps, windows, warm = opt_arg("--steps", 10, int), opt_arg("--windows", 3, int), opt_arg("--warmup", 8, int)
    dev = torch.device("cuda:0")
    H = W = img
    lines = [f"depth supervision, one MI355X: {rays} rays, semi-transparent rays (optical depth 0.1 .. 3), shared depth grid + jitter;",
             f"each entry point on preallocated buffers, 200 back-to-back launches per window (device events), {windows} windows, alternating"]
    for S_ in (64, 128):
        lines += kernel_lines(dev, rays, S_, windows)

    runs = {}
    images = wpts = pts = None
    for on in (False, True):
        torch.manual_seed(42)
        sp = S.make_sys_param(dev, samples=64, scale=2, batch=rays, H=H, W=W, barf_mask=False, precision="f16x3h",
                              **({"depth_weight": LAMBDA} if on else {}))
        model = MC_Model(sp).to(dev)
        S.init_cameras_near_gt(model, noise=1e-3)
        if runs:                    # one workspace pool for both models: their steps never overlap, the keys are the same
            model.nerf.ws_pool = runs[False]["model"].nerf.ws_pool
        model.nerf.reserve_workspaces(rays)
        if images is None:
            images = DeviceImageSet.synthetic(model.train_numb, H, W, dev, seed=7)
            depth = torch.empty(model.train_numb, H * W, device=dev).uniform_(1.0, 8.0)
            depth[torch.rand(model.train_numb, H * W, device=dev) < 0.5] = 0.0
            images = DeviceImageSet(images.images, H, W, depth=depth)
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
        lines.append(f"step  depth_weight {LAMBDA if on else 'off'}: " + "  ".join(f"{x:7.3f}" for x in v) + f"  ms/step   (min {min(v):.3f}, max {max(v):.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
