#!/usr/bin/env python3
"""Step time of the bench workload with the inverse-CDF fine sampler (`fine_sampler = "pdf"`).

    python scripts/time_pdf_sampler.py [--steps K] [--warmup W] [--rays R] [--n-importance I] [--precision P] [--sampler-only]

The workload of bench.py's default line (Ball_Lego-shaped rig, 800x800, coarse 4x128 with 64 samples, fine 8x256, GLOBAL_OPTIM_EPOCH,
one camera per step, R = 32768 rays, f16x3h) with `fine_sampler = "pdf"` and `n_importance` = I: the fine net runs densely on
64 + I depths per ray.  Prints one JSON line: ms per step and rays/s over the timed steps, plus the sampler kernel alone
(HIP events around ops.sample_pdf on the step's shapes).  `--sampler-only` skips the train steps (profiling the kernel).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=32768)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--n-importance", type=int, default=128)
    ap.add_argument("--precision", default="f16x3h")
    ap.add_argument("--img", type=int, default=800)
    ap.add_argument("--sampler-only", action="store_true")
    args = ap.parse_args()

    import torch
    from mc_nerf_amd import ops, synthetic as S
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, RAdam

    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    N, Sc, I = args.rays, args.samples, args.n_importance
    # the sampler kernel alone on the step's shapes
    w = torch.rand(N, Sc, device=dev)
    zgrid = torch.linspace(1.0, 8.0, Sc, device=dev)
    jit = torch.rand(N, device=dev) * 7.0 / Sc
    u = torch.rand(N, I, device=dev)
    for _ in range(3):
        ops.sample_pdf(w, zgrid, jit, u)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        ops.sample_pdf(w, zgrid, jit, u)
    b.record()
    torch.cuda.synchronize()
    rec = {"what": "train step, fine_sampler = pdf", "rays_per_step": N, "samples": Sc, "n_importance": I, "precision": args.precision,
           "sample_pdf_ms": a.elapsed_time(b) / 20}
    if not args.sampler_only:
        H = W = args.img
        sp = S.make_sys_param(dev, samples=Sc, scale=2, batch=N, H=H, W=W, barf_mask=False, precision=args.precision,
                              fine_sampler="pdf", n_importance=I)
        model = MC_Model(sp).to(dev)
        S.init_cameras_near_gt(model, noise=1e-3)
        loss_fn = MC_NeRF_Loss(sp)
        opt = RAdam(model.parameters(), lr=5e-4, weight_decay=4e-4)
        model.nerf.reserve_workspaces(N)
        C = model.train_numb
        wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
        wpts, pts = wpts.to(dev), pts.to(dev)
        images = DeviceImageSet.synthetic(C, H, W, dev, channels=4, seed=7)

        def step(i):
            data = (images, torch.tensor([i % C]), wpts, pts, wpts, pts)
            loss_dict, _, _, _ = model(data, 20, "GLOBAL_OPTIM_EPOCH", 0.6)
            loss = loss_fn(loss_dict, "GLOBAL_OPTIM_EPOCH")
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

        for i in range(args.warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(args.warmup + i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        finite = bool(all(torch.isfinite(p).all() for p in model.parameters()))
        rec.update(steps=args.steps, ms_per_step=dt / args.steps * 1e3, rays_per_s=N * args.steps / dt, fine_rows_per_ray=Sc + I,
                   finite=finite, skipped_optimizer_steps=int(opt.skipped_steps()))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
