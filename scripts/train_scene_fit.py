"""Convergence experiment of fitting the scene box to the voxel sigma cache (`ray_bounds_fit = "voxel"`): does the fitted box
find the scene, how many rays does it skip, what does a step cost, and what does the field learn?

    python scripts/train_scene_fit.py [--steps 500] [--seeds 3] [--out profiles/scene_fit_convergence.txt]        (needs the GPU)

The radiance-field loop is tests/test_y_convergence_gpu._field_run, imported and run as it is (procedural blob scene, 110-camera Ball
rig of radius 3, 100 x 100 float images, 4096 rays per step, 64 x 2 samples, f16x3h), in voxel mode (grid 64^3, 300 dense warm-up
steps: the setting of tests/test_voxel_gpu.py; 100 collapse on this scene) with `ray_bounds_miss = "skip"`; per seed three runs:
  cube   the box is the cube of the grid, +-3.5: the parent's best setting that needs no number from the user;
  hand   the box +-0.9 of scripts/train_ray_skip.py, chosen by hand (it cuts into the blobs' tails);
  fit    `ray_bounds_fit = "voxel"` inside the cube, margin 2 and a refit every 16 calls (the defaults, not tuned).
Reported per run: the box in force at the last step, the share of the training rays skipped over the last 100 steps, the time per training
step (wall clock from step 350 to the last step, all of them past the warm-up, one synchronisation at each end) and the held-out PSNR
(the scene's run-to-run spread is up to 1.7 dB: DESIGN.md 4e)."""
import argparse
import os
import sys
import time
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PRECISION = "f16x3h"
WARMUP, T0_STEP, LAST = 300, 350, 100
VOXEL = dict(coarse_sampler="voxel", grid_nerf=64, voxel_warmup_epoch=WARMUP, ray_bounds="aabb", ray_bounds_miss="skip")
RUNS = {"cube": {}, "hand": dict(ray_bounds_box=(-0.9,) * 3 + (0.9,) * 3), "fit": dict(ray_bounds_fit="voxel")}


def field_run_with(dev, keys, seed, steps):
    """`_field_run(dev, PRECISION, steps, seed)` with `keys` added to its sys_param -> (held-out PSNR, share of the training rays skipped
    over the last LAST steps, ms per training step, the box at the last step, the fit's status or None)."""
    import test_y_convergence_gpu as Y
    import mc_nerf_amd.model as M
    from mc_nerf_amd import synthetic as S
    make, train = S.make_sys_param, M.NeRF_Model.render_rays_train
    acc = {"miss": torch.zeros((), device=dev), "calls": 0, "t0": None, "t1": None, "model": None}

    def render(self, rays_d, rays_o, *a, **kw):
        if acc["calls"] in (T0_STEP, steps - 1):
            torch.cuda.synchronize()
            acc["t0" if acc["calls"] == T0_STEP else "t1"] = time.perf_counter()
        out = train(self, rays_d, rays_o, *a, **kw)
        acc["calls"] += 1
        acc["model"] = self
        if acc["calls"] > steps - LAST:
            acc["miss"] += (self.last_ray_hit == 0).float().mean()
        return out

    with mock.patch.object(S, "make_sys_param", lambda *a, **kw: make(*a, **dict(kw, **keys))), mock.patch.object(M.NeRF_Model, "render_rays_train", render):
        psnr, _, _ = Y._field_run(dev, PRECISION, steps, seed=seed)
    ms = (acc["t1"] - acc["t0"]) / (steps - 1 - T0_STEP) * 1e3 if acc["t0"] is not None and acc["t1"] is not None else float("nan")
    m = acc["model"]
    box = m.scene_box.tolist() if m.settings.fit_box else list(m.settings.box)
    return psnr, float(acc["miss"]) / min(LAST, steps), ms, box, m.scene_box_status() if m.settings.fit_box else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_fit_convergence.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_scene_fit.py trains on the GPU; there is none here")
    dev = torch.device("cuda:0")
    lines = [f"# the scene box fitted to the voxel sigma cache on the blob scene: tests/test_y_convergence_gpu._field_run, 100x100, 4096 rays x {args.steps} steps, 64 x 2 samples, {PRECISION};",
             f"# voxel mode (64^3, {WARMUP} warm-up steps), aabb + skip; cube = the grid's cube, hand = the box +-0.9, fit = ray_bounds_fit \"voxel\" (margin 2, every 16 calls);",
             f"# the box at the last step, share of the training rays skipped (last {LAST} steps), ms per training step (wall clock from step {T0_STEP} to the last),",
             "# held-out PSNR (run-to-run spread of this scene: 1.7 dB)"]
    for seed in range(args.seeds):
        for name, keys in RUNS.items():
            psnr, share, ms, box, status = field_run_with(dev, dict(VOXEL, **keys), seed, args.steps)
            lines.append(f"seed {seed}, {name:4s}: box [{', '.join(f'{v:+.3f}' for v in box)}]" + ("" if status is None else f" (status {status})")
                         + f"; {100 * share:.1f} % skipped; {ms:.2f} ms / step; {psnr:.2f} dB")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
