"""Times the multi-camera train step (`cams_per_step` = K) against the single-camera step at the bench shape: Ball
rig, 110 cameras, 800 x 800, 32768 rays, 64 x 2 samples, f16x3h, one process, random-init selection (bench.py's plain run).

    python scripts/time_multicam.py [out.txt] [--rays N] [--img S] [--steps N] [--ks 1,8,64]        (needs the GPU)

Two measurements, both with device events and nothing but the measured work between them:
  * the full train step (forward, loss, backward, RAdam) for every K: `windows` windows of `steps` steps each, the K's ALTERNATING
    inside every round so that a drift of the machine hits all of them; one model per K, built from the same seed, warmed up first;
  * the ray preamble alone: sample_perm + raygen_fwd + gather_gt (three launches) at K = 1, the fused ray_batch_fwd (one launch) at K > 1.
The question the record answers: does the K = 8 step lie within the spread of the K = 1 windows?
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mc_nerf_amd import ops, synthetic as S  # noqa: E402
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
        sys.exit("time_multicam.py measures on the GPU; there is none here")
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    rays, img = opt_arg("--rays", 32768, int), opt_arg("--img", 800, int)
    steps, windows, warm = opt_arg("--steps", 20, int), opt_arg("--windows", 3, int), opt_arg("--warmup", 8, int)
    ks = [int(v) for v in opt_arg("--ks", "1,8,64", str).split(",")]
    dev = torch.device("cuda:0")
    H = W = img
    runs = {}
    images = wpts = pts = None
    for K in ks:
        torch.manual_seed(42)
        sp = S.make_sys_param(dev, samples=64, scale=2, batch=rays, H=H, W=W, barf_mask=False, precision="f16x3h",
                              **({"cams_per_step": K} if K > 1 else {}))
        model = MC_Model(sp).to(dev)
        S.init_cameras_near_gt(model, noise=1e-3)
        if runs:                    # one workspace pool for all models (~46 GB): their steps never overlap, the keys are the same
            model.nerf.ws_pool = next(iter(runs.values()))["model"].nerf.ws_pool
        model.nerf.reserve_workspaces(rays)
        if images is None:
            images = DeviceImageSet.synthetic(model.train_numb, H, W, dev, channels=4, seed=7)
            wpts, pts = (v.to(dev) for v in S.calibration_points(sp["gt_pose"], sp["intr_mat"][0]))
        runs[K] = dict(model=model, loss=MC_NeRF_Loss(sp), opt=RAdam(model.parameters(), lr=5e-4, weight_decay=4e-4))
    C = runs[ks[0]]["model"].train_numb
    order = torch.randperm(C * 64, generator=torch.Generator().manual_seed(1)) % C          # the camera ids of the steps, host side

    def step_of(K):
        r = runs[K]

        def step(i):
            cams = order[(i * K) % (order.numel() - K):][:K]
            loss_dict, *_ = r["model"]((images, cams, wpts, pts, wpts, pts), 20, "GLOBAL_OPTIM_EPOCH", 0.6)
            loss = r["loss"](loss_dict, "GLOBAL_OPTIM_EPOCH")
            r["opt"].zero_grad(set_to_none=True)
            loss.backward()
            r["opt"].step()
        return step

    def preamble_of(K):
        m = runs[K]["model"]
        with torch.no_grad():
            _, pose, _ = m.add_weights2param(True, True, True)
            kinv = m.intr_inv_adj
        if K == 1:
            p0, k0 = pose[3].contiguous(), kinv[3].contiguous()

            def pre(i):
                pix = ops.sample_perm(H * W, rays, dev)
                ops.raygen_fwd(p0, k0, pix, W)
                ops.gather_gt(images.images[3], pix)
            return pre
        seg, cams = ops.ray_segments(rays, K), order[:K].tolist()
        return lambda i: ops.ray_batch_fwd(pose, kinv, cams, seg, H, W, images=images.images)

    lines = [f"multi-camera step, one MI355X: Ball rig {C} cameras {H}x{W}, {rays} rays, 64x2 samples, f16x3h, random-init selection;",
             f"{windows} windows of {steps} steps per K (device events; the K's alternate inside every round), {warm} warm-up steps each"]
    steps_of = {K: step_of(K) for K in ks}
    for K in ks:
        timed(steps_of[K], warm)
    step_ms = {K: [] for K in ks}
    for w in range(windows):
        for K in ks:
            step_ms[K].append(timed(lambda i: steps_of[K](warm + w * steps + i), steps))
    for K in ks:
        v = step_ms[K]
        lines.append(f"step  K = {K:2d}: " + "  ".join(f"{x:7.3f}" for x in v) + f"  ms/step   (min {min(v):.3f}, max {max(v):.3f})")
    if 1 in step_ms:
        lo, hi = min(step_ms[1]), max(step_ms[1])
        for K in ks:
            if K != 1:
                v = step_ms[K]
                inside = lo <= sum(v) / len(v) <= hi
                lines.append(f"K = {K} mean {sum(v) / len(v):.3f} ms against the K = 1 windows [{lo:.3f}, {hi:.3f}]: "
                             + ("inside their spread" if inside else f"outside by {(sum(v) / len(v) - (hi if sum(v) / len(v) > hi else lo)):+.3f} ms"))
    pres = {K: preamble_of(K) for K in ks}
    for K in ks:
        timed(pres[K], 50)
    pre_us = {K: [] for K in ks}
    for w in range(windows):
        for K in ks:
            pre_us[K].append(1e3 * timed(pres[K], 200))
    for K in ks:
        what = "sample_perm + raygen_fwd + gather_gt (3 launches)" if K == 1 else "ray_batch_fwd (1 launch)"
        lines.append(f"preamble K = {K:2d}: " + "  ".join(f"{x:7.2f}" for x in pre_us[K]) + f"  us   {what}, incl. the ops' output allocations")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
