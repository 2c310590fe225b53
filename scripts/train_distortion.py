"""What the distortion loss (`dist_weight`) does to a short training run of the radiance field.

    python scripts/train_distortion.py [out.txt] [--steps N] [--runs N] [--precision P] [--weights a,b,c]        (needs the GPU)

The loop of scripts/train_mask.py (procedural blob scene, 110-camera Ball rig at 100 x 100, 4096 rays per step, 64 x 2 samples, RAdam
lr 2e-3, five held-out views), with dist_weight in {0, 1e-3, 1e-2, 1e-1}; `runs` seeds each.  Per run:
  sel      the selected share of the fine grid, `last_selection`'s count over rays x 128, mean of the last `TAIL` steps -- what the
           term is meant to move;
  dist_c   mean coarse / fine distortion term over the held-out views' rays, from a jitter-free train-mode render (measured in every
  dist_f   run, the dist_weight = 0 ones included);
  psnr     held-out PSNR of render_rays_test (run-to-run spread of ONE setting: about 1.7 dB, the weight-gradient atomics' order).
Compare against the dist_weight = 0 rows of the same file.  dist_weight has NO tuned default; this records what the values do here.
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mc_nerf_amd import ops, synthetic as S  # noqa: E402
from mc_nerf_amd.model import MC_NeRF_Loss, NeRF_Model, RAdam  # noqa: E402

H = W = 100
N_RAYS = 4096
TAIL = 20


def opt_arg(name, default, cast):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def run(dev, scene, lam, precision, steps, seed):
    pose, Kinv, imgs, train_ids, test_ids = scene
    torch.manual_seed(seed)
    sp = S.make_sys_param(dev, samples=64, scale=2, batch=N_RAYS, H=H, W=W, precision=precision, **({"dist_weight": lam} if lam > 0 else {}))
    model = NeRF_Model(sp).to(dev)
    opt = RAdam(model.parameters(), lr=2e-3, weight_decay=0.0)
    loss_fn = MC_NeRF_Loss(sp)
    cams = torch.randint(len(train_ids), (steps,), generator=torch.Generator().manual_seed(seed)).tolist()
    counts = []
    for step in range(steps):
        i = train_ids[cams[step]]
        pix = torch.randperm(H * W, device=dev)[:N_RAYS]
        d, o = ops.raygen_fwd(pose[i].contiguous(), Kinv[i].contiguous(), pix, W)
        rgb_c, rgb_f = model.render_rays_train(d, o, step, 1.0)
        loss = loss_fn.get_rgb_loss([rgb_c, rgb_f, imgs[i][pix]])
        if lam > 0:
            loss = loss + loss_fn.get_distortion_loss(list(model.last_distortion))
        if step >= steps - TAIL:
            counts.append(model.last_selection[1])          # (device words: read after the loop)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    sel = float(torch.stack(counts).double().mean()) / (N_RAYS * model.samples_f)
    allpix = torch.arange(H * W, device=dev)
    psnr, dc, df, n = [], 0.0, 0.0, 0
    model.dist_weight = 1.0                     # (measurement only: the train-mode render below then keeps its distortion terms)
    with torch.no_grad():
        for i in test_ids:
            d, o = ops.raygen_fwd(pose[i].contiguous(), Kinv[i].contiguous(), allpix, W)
            rgb = model.render_rays_test(d, o, model.nerf_coarse, model.nerf_fine)[0]
            psnr.append(-10 * math.log10(float(((rgb - imgs[i]) ** 2).mean())))
            for lo in range(0, H * W, N_RAYS):
                dd, oo = d[lo:lo + N_RAYS].contiguous(), o[lo:lo + N_RAYS].contiguous()
                model.render_rays_train(dd, oo, steps, 1.0, jitter=torch.zeros(dd.shape[0], 1, device=dev))
                dc += float(model.last_distortion[0].double().sum())
                df += float(model.last_distortion[1].double().sum())
                n += dd.shape[0]
    return sel, dc / n, df / n, sum(psnr) / len(psnr), float(loss.detach())


def main():
    if not torch.cuda.is_available():
        sys.exit("train_distortion.py trains on the GPU; there is none here")
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    steps, runs, precision = opt_arg("--steps", 500, int), opt_arg("--runs", 3, int), opt_arg("--precision", "f16x3", str)
    weights = opt_arg("--weights", (0.0, 1e-3, 1e-2, 1e-1), lambda s: tuple(float(v) for v in s.split(",")))
    dev = torch.device("cuda:0")
    pose, K, _ = S.ball_cameras(seed=0, radius=3.0, H=H, W=W)
    pose, K = pose.to(dev), K.to(dev)
    C = pose.shape[0]
    test_ids = list(range(5, C, 22))
    scene = (pose, torch.linalg.inv(K), S.blob_scene_images(pose, K, H, W), [i for i in range(C) if i not in test_ids], test_ids)
    lines = [f"distortion loss on the procedural blob scene {H}x{W}, {N_RAYS} rays x {steps} steps, 64x2 samples, {precision}, RAdam lr 2e-3, one MI355X;",
             f"held-out views {test_ids}; {runs} seeds per setting; selected share: mean of the last {TAIL} steps",
             "dist_weight  seed   selected share of the fine grid   dist_c held-out   dist_f held-out   psnr dB   last loss"]
    for lam in weights:
        rows = [run(dev, scene, lam, precision, steps, seed) for seed in range(runs)]
        for seed, (s, c, f, p, l) in enumerate(rows):
            lines.append(f"{lam:11.0e}  {seed:4d}   {s:10.4f}   {c:14.4e}   {f:14.4e}   {p:7.2f}   {l:.5f}")
        sel = [r[0] for r in rows]
        lines.append(f"{lam:11.0e}  mean   {sum(sel) / runs:10.4f}   {sum(r[1] for r in rows) / runs:14.4e}   {sum(r[2] for r in rows) / runs:14.4e}   "
                     f"{sum(r[3] for r in rows) / runs:7.2f}   (selected share over the seeds: {min(sel):.4f} .. {max(sel):.4f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
