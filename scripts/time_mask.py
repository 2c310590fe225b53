"""Times the alpha-mask supervision (`mask_weight`) against today's path.

    python scripts/time_mask.py [out.txt] [--rays N] [--img S] [--steps N] [--windows N]        (needs the GPU)

Two measurements, both with device events and nothing but the measured work between them:
  * the kernels alone at N = `rays`, S = 64 and 128 (semi-transparent rays): mcnerf_ext_front_weight beside mcnerf_composite_fwd (the
    train call's form: with selection weights) and mcnerf_ext_composite_bwd_front (with d_fg) beside mcnerf_composite_bwd, plus
    mcnerf_ext_gather_alpha and mcnerf_ext_mask_loss; each entry point on preallocated buffers, alternating inside every round;
  * the full single-camera train step (forward, loss, backward, RAdam) at the bench shape (Ball rig, 110 cameras, 32768 rays,
    64 x 2 samples, f16x3h, random-init selection) with the feature off and on, alternating windows, one model each from one seed.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mc_nerf_amd import _ext, _lib, ops, synthetic as S  # noqa: E402
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


def kernel_lines(dev, rays, S_, windows):
    g = torch.Generator().manual_seed(S_)
    tau = 0.1 + 2.9 * torch.rand(rays, 1, generator=g)
    sig = torch.log(torch.expm1(tau / 7.0)) + 0.3 * torch.randn(rays, S_, generator=g)
    sr = torch.cat([sig.unsqueeze(-1), torch.rand(rays, S_, 3, generator=g)], -1).contiguous().to(dev)
    d = torch.nn.functional.normalize(torch.randn(rays, 3, generator=g), dim=-1).to(dev)
    z, jit = torch.linspace(1, 8, S_).to(dev), (torch.rand(rays, generator=g) * 7.0 / S_).to(dev)
    eps, eps_sel = (0.3 * torch.randn(rays, S_, generator=g)).to(dev), (0.3 * torch.randn(rays, S_, generator=g)).to(dev)
    d_rgb, d_fg = torch.randn(rays, 3, generator=g).to(dev), torch.randn(rays, generator=g).to(dev)
    rgb, w_sel, wmax = torch.empty(rays, 3, device=dev), torch.empty(rays, S_, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    fg, d_out, gmax = torch.empty(rays, device=dev), torch.empty(rays, S_, 4, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    st = ops._stream()
    fns = {
        "composite_fwd": lambda i: _lib.call("mcnerf_composite_fwd", sr, d, z, 0, jit, eps, eps_sel, rays, S_, 1, rgb, None, None, w_sel, wmax, st),
        "ext_front_weight": lambda i: _ext.call("mcnerf_ext_front_weight", sr, z, 0, jit, eps, rays, S_, fg, st),
        "composite_bwd": lambda i: _lib.call("mcnerf_composite_bwd", sr, z, 0, jit, eps, d_rgb, rays, S_, 1, d_out, gmax, st),
        "ext_composite_bwd_front": lambda i: _ext.call("mcnerf_ext_composite_bwd_front", sr, z, 0, jit, eps, d_rgb, d_fg, rays, S_, 1, d_out, gmax, st),
    }
    for f in fns.values():
        timed(f, 50)
    us = {k: [] for k in fns}
    for w in range(windows):
        for k, f in fns.items():
            us[k].append(1e3 * timed(f, 200))
    return [f"S = {S_:3d}  {k:24s}: " + "  ".join(f"{x:7.2f}" for x in v) + f"  us per launch   (min {min(v):.2f})" for k, v in us.items()]


def small_kernel_lines(dev, rays, img, windows):
    C, npix = 8, img * img
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (C, npix, 4), dtype=torch.uint8, generator=g).to(dev)
    pix = torch.randint(0, npix, (rays,), generator=g).to(dev)
    fg_c, fg_f, alpha = (torch.rand(rays, generator=g).to(dev) for _ in range(3))
    d_c, d_f, out = torch.empty_like(fg_c), torch.empty_like(fg_f), torch.zeros(ops.MASK_LOSS_OUT, device=dev)
    st = ops._stream()
    fns = {}
    for K in (1, 8):
        cams, start, _, n = ops._seg_arrays([(3 * k) % C for k in range(K)], ops.ray_segments(rays, K))
        fns[f"ext_gather_alpha K = {K}"] = (lambda cams, start, K: lambda i: _ext.call("mcnerf_ext_gather_alpha", images, C, npix, 4, cams, start, K, pix, rays, alpha, st))(cams, start, K)
    fns["ext_mask_loss"] = lambda i: _ext.call("mcnerf_ext_mask_loss", fg_c, fg_f, alpha, rays, 0.5, out, d_c, d_f, st)
    for f in fns.values():
        timed(f, 50)
    us = {k: [] for k in fns}
    for w in range(windows):
        for k, f in fns.items():
            us[k].append(1e3 * timed(f, 200))
    return [f"         {k:24s}: " + "  ".join(f"{x:7.2f}" for x in v) + f"  us per launch   (min {min(v):.2f})" for k, v in us.items()]


def main():
    if not torch.cuda.is_available():
        sys.exit("time_mask.py measures on the GPU; there is none here")
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    rays, img = opt_arg("--rays", 32768, int), opt_arg("--img", 800, int)
    steps, windows, warm = opt_arg("--steps", 10, int), opt_arg("--windows", 3, int), opt_arg("--warmup", 8, int)
    dev = torch.device("cuda:0")
    H = W = img
    lines = [f"alpha-mask supervision, one MI355X: {rays} rays, semi-transparent rays (optical depth 0.1 .. 3), shared depth grid + jitter;",
             f"each entry point on preallocated buffers, 200 back-to-back launches per window (device events), {windows} windows, alternating"]
    for S_ in (64, 128):
        lines += kernel_lines(dev, rays, S_, windows)
    lines += small_kernel_lines(dev, rays, img, windows)

    runs = {}
    images = wpts = pts = None
    for on in (False, True):
        torch.manual_seed(42)
        sp = S.make_sys_param(dev, samples=64, scale=2, batch=rays, H=H, W=W, barf_mask=False, precision="f16x3h",
                              **({"mask_weight": 0.1} if on else {}))
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
        lines.append(f"step  mask_weight {'0.1' if on else 'off'}: " + "  ".join(f"{x:7.3f}" for x in v) + f"  ms/step   (min {min(v):.3f}, max {max(v):.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
