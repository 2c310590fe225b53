"""Times per-ray sample bounds (`ray_bounds = "aabb"`) against today's path.

    python scripts/time_ray_bounds.py [out.txt] [--rays N] [--img S] [--steps N] [--windows N]        (needs the GPU)

Two measurements, both with device events and nothing but the measured work between them:
  * mcnerf_box_ray_depths alone at N = `rays`, 64 + 128 depths with jitter and the span (what a threshold-mode train call launches), and
    with the coarse grid only (what a pdf-mode call launches), on preallocated buffers; the rays are cameras on a sphere of radius 4
    against the default +-3.5 cube;
  * the full single-camera train step (forward, loss, backward, RAdam) at the bench shape (Ball rig, 110 cameras, 32768 rays,
    64 x 2 samples, f16x3h, random-init selection) with the key off -- "global": the parent commit's path, launch for launch -- and with
    "aabb" and a box that clips nothing (+-1e3): the work of both passes is then identical and the difference is the price of the rows;
    alternating windows of one process, one model each from one seed.  Repeated for fine_sampler = "pdf" and coarse_sampler = "voxel".
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mc_nerf_amd import _box, ops, synthetic as S  # noqa: E402
from mc_nerf_amd.data import DeviceImageSet  # noqa: E402
from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, RAdam  # noqa: E402

NO_CLIP = (-1e3,) * 3 + (1e3,) * 3
CONFIGS = {"threshold / dense": {}, "pdf / dense": {"fine_sampler": "pdf"}, "threshold / voxel": {"coarse_sampler": "voxel", "voxel_warmup_epoch": 0}}


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


def kernel_lines(dev, rays, windows):
    g = torch.Generator().manual_seed(0)
    o = 4.0 * torch.nn.functional.normalize(torch.randn(rays, 3, generator=g), dim=-1)
    d = torch.nn.functional.normalize(torch.randn(rays, 3, generator=g) - o, dim=-1)
    o, d, jit = o.to(dev), d.to(dev), (torch.rand(rays, generator=g) * 7.0 / 64).to(dev)
    zc, zf = torch.linspace(1, 8, 64).to(dev), torch.linspace(1, 8, 128).to(dev)
    z_c, z_f, span = torch.empty(rays, 64, device=dev), torch.empty(rays, 128, device=dev), torch.empty(rays, 2, device=dev)
    box, st = (-3.5,) * 3 + (3.5,) * 3, ops._stream()
    fns = {"box_ray_depths 64 + 128, span": lambda i: _box.call("mcnerf_box_ray_depths", o, d, rays, *box, 1.0, 8.0, jit, zc, 64, zf, 128, z_c, z_f, span, st),
           "box_ray_depths 64, span": lambda i: _box.call("mcnerf_box_ray_depths", o, d, rays, *box, 1.0, 8.0, jit, zc, 64, None, 0, z_c, None, span, st)}
    for f in fns.values():
        timed(f, 50)
    us = {k: [] for k in fns}
    for w in range(windows):
        for k, f in fns.items():
            us[k].append(1e3 * timed(f, 200))
    mb = {"box_ray_depths 64 + 128, span": rays * (192 + 2 + 7) * 4 / 1e6, "box_ray_depths 64, span": rays * (64 + 2 + 7) * 4 / 1e6}
    clipped = float((span[:, 1] - span[:, 0] < 7.0).float().mean())
    lines = [f"{k:30s}: " + "  ".join(f"{x:7.2f}" for x in v) + f"  us per launch   (min {min(v):.2f}: {mb[k] / min(v) * 1e3:.0f} GB/s of {mb[k]:.1f} MB)" for k, v in us.items()]
    return lines + [f"({100 * clipped:.0f} % of these rays are clipped by the +-3.5 cube)"]


def step_lines(dev, rays, img, steps, windows, warm, name, extra):
    H = W = img
    runs = {}
    images = wpts = pts = None
    for mode in ("global", "aabb"):
        torch.manual_seed(42)
        keys = dict(extra, **({"ray_bounds": "aabb", "ray_bounds_box": NO_CLIP} if mode == "aabb" else {}))
        sp = S.make_sys_param(dev, samples=64, scale=2, batch=rays, H=H, W=W, barf_mask=False, precision="f16x3h", **keys)
        model = MC_Model(sp).to(dev)
        S.init_cameras_near_gt(model, noise=1e-3)
        if runs:                    # one workspace pool for both models: their steps never overlap, the keys are the same
            model.nerf.ws_pool = runs["global"]["model"].nerf.ws_pool
        model.nerf.reserve_workspaces(rays)
        if images is None:
            images = DeviceImageSet.synthetic(model.train_numb, H, W, dev, seed=7)
            wpts, pts = (v.to(dev) for v in S.calibration_points(sp["gt_pose"], sp["intr_mat"][0]))
        runs[mode] = dict(model=model, loss=MC_NeRF_Loss(sp), opt=RAdam(model.parameters(), lr=5e-4, weight_decay=4e-4))
    order = torch.randperm(runs["global"]["model"].train_numb * 64, generator=torch.Generator().manual_seed(1)) % runs["global"]["model"].train_numb

    def step_of(mode):
        q = runs[mode]

        def step(i):
            loss_dict, *_ = q["model"]((images, order[i:i + 1], wpts, pts, wpts, pts), 20, "GLOBAL_OPTIM_EPOCH", 0.6)
            loss = q["loss"](loss_dict, "GLOBAL_OPTIM_EPOCH")
            q["opt"].zero_grad(set_to_none=True)
            loss.backward()
            q["opt"].step()
        return step

    steps_of = {mode: step_of(mode) for mode in runs}
    for mode in runs:
        timed(steps_of[mode], warm)
    ms = {mode: [] for mode in runs}
    for w in range(windows):
        for mode in runs:
            ms[mode].append(timed(lambda i: steps_of[mode](warm + w * steps + i), steps))
    lines = [f"full train step, {name}: Ball rig {H}x{W}, {rays} rays, 64x2 samples, f16x3h, random-init selection; {windows} windows of {steps} steps, alternating:"]
    for mode in runs:
        v = ms[mode]
        lines.append(f"step  ray_bounds {mode:6s}: " + "  ".join(f"{x:7.3f}" for x in v) + f"  ms/step   (min {min(v):.3f}, max {max(v):.3f})")
    return lines


def main():
    if not torch.cuda.is_available():
        sys.exit("time_ray_bounds.py measures on the GPU; there is none here")
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    rays, img = opt_arg("--rays", 32768, int), opt_arg("--img", 800, int)
    steps, windows, warm = opt_arg("--steps", 20, int), opt_arg("--windows", 3, int), opt_arg("--warmup", 8, int)
    dev = torch.device("cuda:0")
    lines = [f"per-ray sample bounds, one MI355X: {rays} rays; the entry point on preallocated buffers, 200 back-to-back launches per window (device events), "
             f"{windows} windows, alternating"]
    lines += kernel_lines(dev, rays, windows)
    lines.append('"global" is this build with the key off: the parent commit\'s path, launch for launch (nothing is allocated, the bounds library is not loaded for it);')
    lines.append('"aabb" runs on a box that clips nothing (+-1e3): the same samples, the difference is the price of the rows')
    for name, extra in CONFIGS.items():
        lines += step_lines(dev, rays, img, steps, windows, warm, name, extra)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
