#!/usr/bin/env python3
"""Step time of the bench workload with the voxel sigma cache (`coarse_sampler = "voxel"`) against the dense coarse pass.

    python scripts/time_voxel_coarse.py [--steps K] [--warmup W] [--rays R] [--out FILE]

The workload of bench.py's default line (Ball_Lego-shaped rig, 800x800, coarse 4x128 with 64 samples, fine 8x256 with 128,
GLOBAL_OPTIM_EPOCH, one camera per step, R = 32768 rays, f16x3h), G = 384.  In voxel mode the grid is set to a centred ball (+5 inside,
-5 outside) whose radius is searched so that the coarse list is ~5 % and ~25 % of N * Sc on the step's own rays; voxel_beta is 1e-6, so the
update kernels run at their full cost while the list stays what the search found (the fractions at the start and the end of each window
are printed).  Timed in one process, in this order:
  1. the train step in dense mode, three windows: their spread is the margin a difference must exceed to be called one;
  2. the train step in voxel mode at each fraction;
  3. the coarse pass alone, forward + backward (render_rays_train(only_coarse=True) and its loss), dense and at each fraction: the part of
     the step the list changes, free of the fine pass (in (2) the pruned samples carry sigma_default, so the fine list shrinks with the
     coarse one, which a random-init dense run does not share: (2) flatters voxel mode, (3) does not);
  4. the new kernels on their own (HIP events around the ops, as scripts/time_kernels.py times its kernels).
Writes the table to --out (default profiles/voxel_coarse_step.txt) and prints it.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G, PRECISION, SC = 384, "f16x3h", 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=32768)
    ap.add_argument("--img", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "voxel_coarse_step.txt"))
    args = ap.parse_args()

    import torch
    from mc_nerf_amd import ops, synthetic as S
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, RAdam

    dev = torch.device("cuda:0")
    N, H, W = args.rays, args.img, args.img
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def make(**kw):
        torch.manual_seed(42)
        sp = S.make_sys_param(dev, samples=SC, scale=2, batch=N, H=H, W=W, barf_mask=False, precision=PRECISION, **kw)
        model = MC_Model(sp).to(dev)
        S.init_cameras_near_gt(model, noise=1e-3)
        model.nerf.reserve_workspaces(N)
        return model, sp

    def ball(nerf, radius):
        a =((torch.arange(G, dtype=torch.float32, device=dev) + 0.5) * ((nerf.boader_max - nerf.boader_min) / G) + nerf.boader_min) ** 2
        r2 = a[:, None, None] + a[None, :, None] + a[None, None, :]
        nerf.sigma_voxels.copy_(torch.where(r2 < radius * radius, 5.0, -5.0))

    def fraction(nerf, d, o):
        _, count, _ = ops.voxel_select(nerf.voxel_grid(), nerf.settings.voxel_thresh, o, d, nerf.z_vals_c, None, nerf.sigma_default, prefill=False)
        return int(count.item()) / (d.shape[0] * SC)

    def search_radius(nerf, d, o, target):
        lo, hi = 0.0, 7.0
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            ball(nerf, mid)
            lo, hi = (mid, hi) if fraction(nerf, d, o) < target else (lo, mid)
        ball(nerf, hi)
        return hi, fraction(nerf, d, o)

    def window(fn):
        for i in range(args.warmup):
            fn(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            fn(args.warmup + i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    def stepper(model, sp):
        loss_fn = MC_NeRF_Loss(sp)
        opt = RAdam(model.parameters(), lr=5e-4, weight_decay=4e-4)
        wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
        wpts, pts = wpts.to(dev), pts.to(dev)
        images = DeviceImageSet.synthetic(model.train_numb, H, W, dev, channels=4, seed=7)

        def step(i):
            data = (images, torch.tensor([i % model.train_numb]), wpts, pts, wpts, pts)
            loss_dict, _, _, _ = model(data, 20, "GLOBAL_OPTIM_EPOCH", 0.6)
            loss = loss_fn(loss_dict, "GLOBAL_OPTIM_EPOCH")
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return step

    def coarse_only(model, d, o, gt):
        def step(i):
            for p in model.nerf.parameters():
                p.grad = None
            rgb_c, _, _ = model.nerf.render_rays_train(d, o, 20, 0.6, only_coarse=True)
            ((rgb_c - gt) ** 2).mean().backward()
        return step

    def fine_fraction(nerf):
        sel = nerf.last_selection
        return float("nan") if sel is None else int(sel[1].item()) / (N * nerf.samples_f)

    # the rays of the coarse-only windows, the radius search and the kernel timings: one camera of the rig, as a step draws them
    g = torch.Generator(device=dev).manual_seed(0)
    o = torch.nn.functional.normalize(torch.randn(N, 3, device=dev, generator=g), dim=-1) * 3
    d = torch.nn.functional.normalize(-o + 0.5 * torch.randn(N, 3, device=dev, generator=g), dim=-1)
    gt = torch.rand(N, 3, device=dev, generator=g)

    say(f"voxel sigma cache against the dense coarse pass: {N} rays x ({SC} + {2 * SC}) samples, coarse 4x128, fine 8x256, {PRECISION}, G = {G}, "
        f"{args.steps} steps per window after {args.warmup} warm-up steps, one process")
    say()
    # ---- 1. dense, three windows
    model, sp = make()
    step = stepper(model, sp)
    dense = [window(step) for _ in range(3)]
    spread = max(dense) - min(dense)
    say(f"train step, dense (three windows)        {dense[0]:8.3f} {dense[1]:8.3f} {dense[2]:8.3f} ms   spread {spread:.3f} ms   fine list {fine_fraction(model.nerf):.3f} of N * Sf")
    dense_c = [window(coarse_only(model, d, o, gt)) for _ in range(3)]
    spread_c = max(dense_c) - min(dense_c)
    del model, step
    torch.cuda.empty_cache()
    # ---- 2. / 3. voxel mode at each fraction
    model, sp = make(coarse_sampler="voxel", grid_nerf=G, voxel_warmup_epoch=0, voxel_beta=1e-6)
    nerf = model.nerf
    step = stepper(model, sp)
    coarse_rows, kernel_rows = [], []
    for target in (0.05, 0.25):
        radius, f0 = search_radius(nerf, d, o, target)
        ms = window(step)
        f_step = int(nerf.last_coarse_selection[1].item()) / (N * SC)
        say(f"train step, voxel, ball radius {radius:5.3f}        {ms:8.3f} ms   dense - voxel = {min(dense) - ms:+.3f} .. {max(dense) - ms:+.3f} ms   "
            f"coarse list {f_step:.3f} of N * Sc on the last step's rays ({f0:.3f} on the search rays)   fine list {fine_fraction(nerf):.3f} of N * Sf")
        ms_c = window(coarse_only(model, d, o, gt))
        coarse_rows.append(f"coarse pass fwd + bwd alone, voxel, list {fraction(nerf, d, o):.3f}   {ms_c:8.3f} ms   dense - voxel = {min(dense_c) - ms_c:+.3f} .. {max(dense_c) - ms_c:+.3f} ms")
        # ---- 4. the kernels on their own, on this list
        grid, jit = nerf.voxel_grid(), torch.rand(N, device=dev) * 7.0 / SC
        idx, count, out_c = ops.voxel_select(grid, 0.0, o, d, nerf.z_vals_c, jit, nerf.sigma_default)
        out_c[..., 0] = torch.randn(N, SC, device=dev)
        pts = (o.unsqueeze(1) + d.unsqueeze(1) * nerf.z_vals_c.reshape(1, -1, 1)).reshape(-1, 3).contiguous()
        sig = out_c[..., 0].reshape(-1).contiguous()
        fns = {"select": lambda: ops.voxel_select(grid, 0.0, o, d, nerf.z_vals_c, jit, nerf.sigma_default),
               "update, listed": lambda: ops.voxel_update(grid, 1e-6, o, d, nerf.z_vals_c, jit, out_c, idx, count, N * SC),
               "update, all N * Sc": lambda: ops.voxel_update(grid, 1e-6, o, d, nerf.z_vals_c, jit, out_c),
               f"query, {N * SC} points": lambda: ops.voxel_query(grid, pts),
               f"update_points, {N * SC} points": lambda: ops.voxel_update_points(grid, pts, sig, 1e-6)}
        for name, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            kernel_rows.append(f"  list {int(count.item()) / (N * SC):.3f}   {name:34s} {e0.elapsed_time(e1) / 20 * 1e3:9.1f} us  (its launches and the wrapper's allocations included)")
    say()
    say(f"coarse pass fwd + bwd alone, dense (three windows)  {dense_c[0]:8.3f} {dense_c[1]:8.3f} {dense_c[2]:8.3f} ms   spread {spread_c:.3f} ms")
    for r in coarse_rows:
        say(r)
    say()
    say("the new ops on their own (20 calls between two HIP events):")
    for r in kernel_rows:
        say(r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
