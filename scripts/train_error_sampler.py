"""Effect experiment of the error-guided pixel sampler: does drawing pixels in proportion to a running per-tile error
change what the field reaches in a fixed number of steps?

    python scripts/train_error_sampler.py [--steps 500] [--runs 3] [--tile 16] [--beta 0.5] [--frac 0.5] [--out profiles/error_sampler_convergence.txt]

The loop is that of tests/test_y_convergence_gpu._field_run (procedural blob scene on white, 110-camera Ball rig, 100 x 100 float
images, 4096 rays per step, f16x3h, RAdam lr 2e-3, the step's camera from a host-side draw), restated here because the pixel draw sits
in its middle; the ops are driven directly beside NeRF_Model:
  uniform  pix = randperm(H W)[:4096], the loop's own draw (without replacement);
  error    pix = ops.errmap_sample(map, [cam], [0, 4096], frac) (with replacement), and after the render
           ops.errmap_update(map, [cam], [0, 4096], pix, rgb_f, gt, beta).
Both from the same seeds, `runs` runs each.  Reported per run: the held-out PSNR (five cameras never trained on, all pixels) and the share
of the LAST step's rays that fall in tiles whose clean image is pure background (every pixel within 1e-3 of white).  The tile size,
beta and the uniform fraction are the keys' defaults: starting values, not tuned."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H = W = 100
N_RAYS = 4096
PRECISION = "f16x3h"


def field_run(dev, mode, steps, seed=0, tile=16, beta=0.5, frac=0.5):
    """-> (held-out PSNR, share of the last step's rays in pure-background tiles)."""
    from mc_nerf_amd import ops, synthetic as S
    from mc_nerf_amd.model import MC_NeRF_Loss, NeRF_Model, RAdam
    torch.manual_seed(seed)
    pose, K, _ = S.ball_cameras(seed=0, radius=3.0, H=H, W=W)
    pose, K = pose.to(dev), K.to(dev)
    Kinv = torch.linalg.inv(K)
    C = pose.shape[0]
    imgs = S.blob_scene_images(pose, K, H, W)
    test_ids = list(range(5, C, 22))
    train_ids = [i for i in range(C) if i not in test_ids]
    sp = S.make_sys_param(dev, samples=64, scale=2, batch=N_RAYS, H=H, W=W, precision=PRECISION)
    model = NeRF_Model(sp).to(dev)
    opt = RAdam(model.parameters(), lr=2e-3, weight_decay=0.0)
    loss_fn = MC_NeRF_Loss(sp)
    allpix = torch.arange(H * W, device=dev)
    cams = torch.randint(len(train_ids), (steps,), generator=torch.Generator().manual_seed(seed)).tolist()
    emap = ops.ErrorMap(C, H, W, tile, dev) if mode == "error" else None
    pix = i = None
    for step in range(steps):
        i = train_ids[cams[step]]
        if emap is None:
            pix = torch.randperm(H * W, device=dev)[:N_RAYS]
        else:
            pix = ops.errmap_sample(emap, [i], [0, N_RAYS], frac)
        d, o = ops.raygen_fwd(pose[i].contiguous(), Kinv[i].contiguous(), pix, W)
        rgb_c, rgb_f = model.render_rays_train(d, o, step, 1.0)
        gt = imgs[i][pix]
        loss = loss_fn.get_rgb_loss([rgb_c, rgb_f, gt])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        if emap is not None:
            ops.errmap_update(emap, [i], [0, N_RAYS], pix, rgb_f.detach().contiguous(), gt.contiguous(), beta)
    assert int(opt.skipped_steps()) == 0
    # tiles of the last step's camera whose clean image is pure background
    Th, Tw = -(-H // tile), -(-W // tile)
    tile_id = (allpix // W) // tile * Tw + (allpix % W) // tile
    off_white = (1.0 - imgs[i]).abs().amax(-1)
    worst = torch.zeros(Th * Tw, device=dev).scatter_reduce(0, tile_id, off_white, "amax")
    share = float((worst[tile_id[pix]] < 1e-3).float().mean())
    bg_area = float((worst[tile_id] < 1e-3).float().mean())
    vals = []
    with torch.no_grad():
        for t in test_ids:
            d, o = ops.raygen_fwd(pose[t].contiguous(), Kinv[t].contiguous(), allpix, W)
            rgb = model.render_rays_test(d, o, model.nerf_coarse, model.nerf_fine)[0]
            vals.append(-10 * math.log10(float(((rgb - imgs[t]) ** 2).mean())))
    return sum(vals) / len(vals), share, bg_area


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tile", type=int, default=16)
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--frac", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_sampler_convergence.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# error-guided pixel sampling on the procedural scene: {H}x{W}, {N_RAYS} rays x {args.steps} steps, {PRECISION}, tile {args.tile}, "
             f"error_beta {args.beta:g}, error_uniform_frac {args.frac:g} (the defaults: starting values, not tuned); seed 0 every run (runs",
             "# differ by the order of the weight-gradient atomics; repeated runs of one configuration differ by up to 1.7 dB here:",
             "# tests/test_y_convergence_gpu.py).  background share: the LAST step's rays in tiles whose clean image is pure background",
             "# (in brackets: the share of the image those tiles cover, i.e. what a uniform draw expects)"]
    res = {"uniform": [], "error": []}
    for run in range(args.runs):
        for mode in ("uniform", "error"):
            psnr, share, area = field_run(dev, mode, args.steps, tile=args.tile, beta=args.beta, frac=args.frac)
            res[mode].append(psnr)
            lines.append(f"run {run + 1} {mode:7s}: held-out PSNR {psnr:.2f} dB, background share of the last step's rays {share:.3f} (tiles cover {area:.3f})")
            print(lines[-1], flush=True)
    mean = {m: sum(v) / len(v) for m, v in res.items()}
    spread = max(max(v) - min(v) for v in res.values())
    lines.append(f"mean uniform {mean['uniform']:.2f} dB, error {mean['error']:.2f} dB, difference {mean['error'] - mean['uniform']:+.2f} dB; "
                 f"largest run-to-run spread of one configuration here {spread:.2f} dB")
    print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
