"""Convergence experiment of per-ray sample bounds (`ray_bounds = "aabb"`): at equal cost, do the samples that clipping
moves out of empty space buy quality on the blob scene?

    python scripts/train_ray_bounds.py [--steps 500] [--seeds 3] [--out profiles/ray_bounds_convergence.txt]        (needs the GPU)

The radiance-field loop is tests/test_y_convergence_gpu._field_run, imported and run as it is (procedural blob scene, 110-camera Ball
rig of radius 3, 100 x 100 float images, 4096 rays per step, 64 x 2 samples, f16x3h); per seed three runs:
  global   today's path;
  cube     aabb with the default cube [boader_min, boader_max]^3 = +-3.5 (the cameras sit inside it: only the far end is clipped);
  fit      aabb with the box +-1.8: every blob centre of mc_nerf_amd/synthetic.py (|c| <= 0.5 per axis) with four of the largest blob's
           standard deviations (0.32) of margin; the density outside is below 18 exp(-8) = 0.006.
Reported per run: the held-out PSNR (the scene's run-to-run spread is up to 1.7 dB: DESIGN.md 4e), the mean hi - lo of the training rays
and the share of them that the box clips.  With `--voxel` the same three runs in coarse_sampler = "voxel" mode, one seed, which also
report the share of the N * Sc coarse samples that were listed."""
import argparse
import os
import sys
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PRECISION = "f16x3h"
FIT = (-1.8,) * 3 + (1.8,) * 3
MODES = {"global": {}, "cube": {"ray_bounds": "aabb"}, "fit": {"ray_bounds": "aabb", "ray_bounds_box": FIT}}


def field_run_with(dev, keys, seed, steps):
    """`_field_run(dev, PRECISION, steps, seed)` with `keys` added to its sys_param -> (held-out PSNR, mean hi - lo of the training
    rays | None, share of them clipped | None, share of the coarse samples listed | None); the sums stay on the device until the end."""
    import test_y_convergence_gpu as Y
    import mc_nerf_amd.model as M
    from mc_nerf_amd import synthetic as S
    make, train = S.make_sys_param, M.NeRF_Model.render_rays_train
    acc = {"span": torch.zeros((), device=dev), "clipped": torch.zeros((), device=dev), "listed": torch.zeros((), device=dev), "calls": 0, "voxel": False}

    def render(self, rays_d, rays_o, *a, **kw):
        out = train(self, rays_d, rays_o, *a, **kw)
        acc["calls"] += 1
        if self.last_ray_span is not None:
            w = self.last_ray_span[:, 1] - self.last_ray_span[:, 0]
            acc["span"] += w.mean()
            acc["clipped"] += (w < self.far - self.near).float().mean()
        if self.last_coarse_selection is not None:
            acc["voxel"] = True
            acc["listed"] += self.last_coarse_selection[1].float().sum() / (rays_d.shape[0] * self.samples_c)
        return out

    with mock.patch.object(S, "make_sys_param", lambda *a, **kw: make(*a, **dict(kw, **keys))), mock.patch.object(M.NeRF_Model, "render_rays_train", render):
        psnr, _, _ = Y._field_run(dev, PRECISION, steps, seed=seed)
    n = max(acc["calls"], 1)
    aabb = keys.get("ray_bounds") == "aabb"
    return psnr, float(acc["span"]) / n if aabb else None, float(acc["clipped"]) / n if aabb else None, float(acc["listed"]) / n if acc["voxel"] else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--voxel", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_bounds_convergence.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_ray_bounds.py trains on the GPU; there is none here")
    dev = torch.device("cuda:0")
    lines = [f"# per-ray sample bounds on the blob scene: tests/test_y_convergence_gpu._field_run, 100x100, 4096 rays x {args.steps} steps, 64 x 2 samples, {PRECISION};",
             f"# cube = aabb on +-3.5 (the default), fit = aabb on +-1.8; held-out PSNR (run-to-run spread of this scene: 1.7 dB), mean hi - lo and clipped share of the training rays"]
    configs = [("", {}, list(range(args.seeds)))] + ([("voxel ", {"coarse_sampler": "voxel"}, [0])] if args.voxel else [])
    for tag, extra, seeds in configs:
        for seed in seeds:
            parts = []
            for mode, keys in MODES.items():
                psnr, span, clipped, listed = field_run_with(dev, dict(extra, **keys), seed, args.steps)
                parts.append(f"{mode} {psnr:.2f} dB" + ("" if span is None else f" (hi - lo {span:.2f}, {100 * clipped:.0f} % clipped)")
                             + ("" if listed is None else f" [{100 * listed:.1f} % of N Sc listed]"))
            lines.append(f"{tag}seed {seed}: " + "; ".join(parts))
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
