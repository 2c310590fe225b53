"""Times the error-guided pixel sampler (`pixel_sampler` = "error").

    python scripts/time_error_sampler.py [out.txt] [--rays N] [--img S] [--tile T] [--steps N] [--windows N]        (needs the GPU)

Two measurements, both with device events and nothing but the measured work between them:
  * the two entry points alone at N = `rays`, an `img` x `img` image, tile `tile`, K = 1 / 8 / 64: mcnerf_errmap_sample (CDF + draw, two
    launches) and mcnerf_errmap_update (max + blend, two launches) on preallocated buffers, next to mcnerf_sample_perm (the uniform
    draw they replace), alternating inside every round;
  * the full train step (forward, loss, backward, RAdam) at the bench shape (Ball rig, 110 cameras, 32768 rays, 64 x 2 samples,
    f16x3h, random-init selection) with the feature off and on, alternating windows, one model each from one seed: the single-camera
    step, the same with color_calib = "affine" (the map then learns the corrected colours), and the 64-camera step with it.
    At random init the nets explain nothing, so this is the cost of the feature's launches, not of what it draws later in training.
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
        sys.exit("time_error_sampler.py measures on the GPU; there is none here")
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    rays, img, tile = opt_arg("--rays", 32768, int), opt_arg("--img", 800, int), opt_arg("--tile", 16, int)
    steps, windows, warm = opt_arg("--steps", 20, int), opt_arg("--windows", 3, int), opt_arg("--warmup", 8, int)
    dev = torch.device("cuda:0")
    H = W = img
    C = 110
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    em = ops.ErrorMap(C, H, W, tile, dev)
    em.err.copy_(r(C, em.Th, em.Tw))
    u, rgb, gt = r(rays, 2), r(rays, 3), r(rays, 3)
    pix = torch.empty(rays, dtype=torch.int64, device=dev)
    perm_out = torch.empty(rays, dtype=torch.int64, device=dev)
    seed = torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int32, device=dev)
    st = ops._stream()
    beta, omb = ops.voxel_blend(0.5)

    def perm(i):
        _lib.call("mcnerf_sample_perm", perm_out, H * W, rays, seed, st)

    def pair_of(K):
        cams, start, _, n = ops._seg_arrays([(7 * k) % C for k in range(K)], ops.ray_segments(rays, K))

        def sample(i):
            _lib.call("mcnerf_errmap_sample", em.err, C, H, W, tile, cams, start, K, n, 0.5, u, em.cdf, pix, st)

        def update(i):
            _lib.call("mcnerf_errmap_update", em.err, em.scratch, C, H, W, tile, cams, start, K, n, pix, rgb, gt,
                      beta, omb, st)
        return sample, update

    fns = {"sample_perm": perm}
    for K in (1, 8, 64):
        fns[f"errmap_sample K = {K:2d}"], fns[f"errmap_update K = {K:2d}"] = pair_of(K)
    for f in fns.values():
        timed(f, 50)
    us = {k: [] for k in fns}
    for w in range(windows):
        for k, f in fns.items():
            us[k].append(1e3 * timed(f, 200))
    lines = [f"error-guided pixel sampler, one MI355X: {rays} rays, {C} cameras of {H}x{W}, tile {tile} ({em.Th * em.Tw} tiles per camera);",
             f"each entry point on preallocated buffers (errmap_*: two launches each), 200 back-to-back calls per window (device events), {windows} windows, alternating"]
    for k, v in us.items():
        lines.append(f"{k:22s}: " + "  ".join(f"{x:7.2f}" for x in v) + f"  us per call   (min {min(v):.2f})")

    err_keys, affine = {"pixel_sampler": "error", "error_tile": tile}, {"color_calib": "affine"}
    configs = {"K =  1  uniform": (1, {}), "K =  1  error": (1, err_keys),
               "K =  1  uniform + affine": (1, affine), "K =  1  error + affine": (1, {**err_keys, **affine}),
               "K = 64  uniform + affine": (64, affine), "K = 64  error + affine": (64, {**err_keys, **affine})}
    runs = {}
    images = wpts = pts = None
    for name, (K, extra) in configs.items():
        torch.manual_seed(42)
        sp = S.make_sys_param(dev, samples=64, scale=2, batch=rays, H=H, W=W, barf_mask=False, precision="f16x3h",
                              **({"cams_per_step": K} if K > 1 else {}), **extra)
        model = MC_Model(sp).to(dev)
        S.init_cameras_near_gt(model, noise=1e-3)
        if "color_calib" in extra:          # a non-zero correction, so that the map's corrected colours differ from the render
            with torch.no_grad():
                model.weights_color.copy_(0.2 * torch.rand(model.train_numb, 6, generator=torch.Generator().manual_seed(8)) - 0.1)
        if runs:                    # one workspace pool for all models: their steps never overlap, the keys are the same
            model.nerf.ws_pool = next(iter(runs.values()))["model"].nerf.ws_pool
        model.nerf.reserve_workspaces(rays)
        if "pixel_sampler" in extra:
            model.reserve_error_map()
        if images is None:
            images = DeviceImageSet.synthetic(model.train_numb, H, W, dev, channels=4, seed=7)
            wpts, pts = (v.to(dev) for v in S.calibration_points(sp["gt_pose"], sp["intr_mat"][0]))
        runs[name] = dict(K=K, model=model, loss=MC_NeRF_Loss(sp), opt=RAdam(model.parameters(), lr=5e-4, weight_decay=4e-4))
    n_cam = next(iter(runs.values()))["model"].train_numb
    order = torch.randperm(n_cam * 64, generator=torch.Generator().manual_seed(1)) % n_cam      # the camera ids of the steps, host side

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
    lines.append("alternating; K = cams_per_step, affine = color_calib (the map then learns the corrected colours: three more torch launches at K = 1, five at any K > 1):")
    for name, v in ms.items():
        lines.append(f"step  {name:25s}: " + "  ".join(f"{x:7.3f}" for x in v) + f"  ms/step   (min {min(v):.3f}, max {max(v):.3f})")
    for off, on in (("K =  1  uniform", "K =  1  error"), ("K =  1  uniform + affine", "K =  1  error + affine"),
                    ("K = 64  uniform + affine", "K = 64  error + affine")):
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
