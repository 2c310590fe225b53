"""Convergence experiment of skipping the rays that miss the scene box (`ray_bounds_miss = "skip"`): does not evaluating
them change what the field learns, and what does a step cost?

    python scripts/train_ray_skip.py [--steps 500] [--seeds 3] [--out profiles/ray_skip_convergence.txt]        (needs the GPU)

The radiance-field loop is tests/test_y_convergence_gpu._field_run, imported and run as it is (procedural blob scene, 110-camera Ball
rig of radius 3, 100 x 100 float images, 4096 rays per step, 64 x 2 samples, f16x3h), in aabb mode on the box +-1.8 of
scripts/train_ray_bounds.py ("fit") and, so that a part of the rays does miss, on +-0.9 ("tight": it cuts into the blobs' tails); per
seed and box two runs, "sample" and "skip".  Reported per run: the held-out PSNR (the scene's run-to-run spread is up to 1.7 dB:
DESIGN.md 4e), the share of the training rays that miss the box, and the time per training step (wall clock between step 50 and the
last step, one synchronisation at each end)."""
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
BOXES = {"fit +-1.8": (-1.8,) * 3 + (1.8,) * 3, "tight +-0.9": (-0.9,) * 3 + (0.9,) * 3}
T0_STEP = 50


def field_run_with(dev, keys, seed, steps):
    """`_field_run(dev, PRECISION, steps, seed)` with `keys` added to its sys_param -> (held-out PSNR, share of the training rays that
    miss the box, ms per training step); the sum stays on the device until the end."""
    import test_y_convergence_gpu as Y
    import mc_nerf_amd.model as M
    from mc_nerf_amd import ops, synthetic as S
    make, train = S.make_sys_param, M.NeRF_Model.render_rays_train
    acc = {"miss": torch.zeros((), device=dev), "calls": 0, "t0": None, "t1": None}

    def render(self, rays_d, rays_o, *a, **kw):
        if acc["calls"] in (T0_STEP, steps - 1):
            torch.cuda.synchronize()
            acc["t0" if acc["calls"] == T0_STEP else "t1"] = time.perf_counter()
        out = train(self, rays_d, rays_o, *a, **kw)
        acc["calls"] += 1
        hit = self.last_ray_hit
        if hit is None:                                     # "sample": the same flags, from a launch of their own
            hit = ops.ray_depths(rays_o, rays_d, self.settings.box, self.near, self.far, None, self.z_vals_c, want_span=False, want_hit=True)[3]
        acc["miss"] += (hit == 0).float().mean()
        return out

    with mock.patch.object(S, "make_sys_param", lambda *a, **kw: make(*a, **dict(kw, **keys))), mock.patch.object(M.NeRF_Model, "render_rays_train", render):
        psnr, _, _ = Y._field_run(dev, PRECISION, steps, seed=seed)
    ms = (acc["t1"] - acc["t0"]) / (steps - 1 - T0_STEP) * 1e3 if acc["t0"] is not None and acc["t1"] is not None else float("nan")
    return psnr, float(acc["miss"]) / max(acc["calls"], 1), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_skip_convergence.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_ray_skip.py trains on the GPU; there is none here")
    dev = torch.device("cuda:0")
    lines = [f"# skipping the rays that miss the box on the blob scene: tests/test_y_convergence_gpu._field_run, 100x100, 4096 rays x {args.steps} steps, 64 x 2 samples, {PRECISION};",
             "# aabb mode, \"sample\" against \"skip\"; held-out PSNR (run-to-run spread of this scene: 1.7 dB), share of the training rays that miss the box,",
             f"# ms per training step (wall clock from step {T0_STEP} to the last; the \"sample\" runs launch ray_depths a second time for the share)"]
    for name, box in BOXES.items():
        for seed in range(args.seeds):
            parts = []
            for miss in ("sample", "skip"):
                psnr, share, ms = field_run_with(dev, dict(ray_bounds="aabb", ray_bounds_box=box, ray_bounds_miss=miss), seed, args.steps)
                parts.append(f"{miss} {psnr:.2f} dB ({100 * share:.1f} % miss, {ms:.2f} ms / step)")
            lines.append(f"{name}, seed {seed}: " + "; ".join(parts))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
