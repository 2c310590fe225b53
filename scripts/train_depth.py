"""What the depth term (`depth_weight`) does to a short training run of the radiance field.

    python scripts/train_depth.py [out.txt] [--steps N] [--runs N] [--precision P]        (needs the GPU)

The loop of tests/test_y_convergence_gpu.py::_field_run (procedural blob scene, 110-camera Ball rig at 100 x 100, 4096 rays per step,
64 x 2 samples, RAdam lr 2e-3, five held-out views), with depth_weight in {0, 0.1, 1} and the scene's analytic depth
(synthetic.blob_scene_depth_images: ray distance where alpha >= 0.5, else no measurement) as the target; `runs` seeds each.  Per run:
  psnr     held-out PSNR of render_rays_test (run-to-run spread of ONE setting: up to 1.7 dB, the weight-gradient atomics' order);
  depth    held-out mean |depth - analytic depth| of render_rays_test's reference `depth` output over the pixels that have a target;
  opac     held-out mean opacity of render_rays_test over those pixels (an empty scene has none);
  sel      the selected share of the fine grid (count / (rays x 128)), mean of the last 20 steps;
  empty    the run ended at the empty scene: held-out opacity on the object below 0.5.
depth_weight has NO tuned default; this records what three values do here, nothing more.
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


def opt_arg(name, default, cast):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def run(dev, scene, lam, precision, steps, seed):
    pose, Kinv, imgs, depths, train_ids, test_ids = scene
    torch.manual_seed(seed)
    sp = S.make_sys_param(dev, samples=64, scale=2, batch=N_RAYS, H=H, W=W, precision=precision, **({"depth_weight": lam} if lam > 0 else {}))
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
            loss = loss + loss_fn.get_depth_loss([*model.last_expected_depth, depths[i][pix]], model.near, model.far)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        if step >= steps - 20:
            counts.append(model.last_selection[1])              # (device words: read after the loop)
    sel = sum(float(c.item()) for c in counts) / (len(counts) * N_RAYS * model.samples_f)
    allpix = torch.arange(H * W, device=dev)
    psnr, err, opac, n = [], 0.0, 0.0, 0
    with torch.no_grad():
        for i in test_ids:
            d, o = ops.raygen_fwd(pose[i].contiguous(), Kinv[i].contiguous(), allpix, W)
            rgb, depth, opacity = model.render_rays_test(d, o, model.nerf_coarse, model.nerf_fine)
            psnr.append(-10 * math.log10(float(((rgb - imgs[i]) ** 2).mean())))
            ok = depths[i] > 0
            err += float((depth.reshape(-1)[ok] - depths[i][ok]).abs().double().sum())
            opac += float(opacity.reshape(-1)[ok].double().sum())
            n += int(ok.sum())
    return sum(psnr) / len(psnr), err / max(n, 1), opac / max(n, 1), sel, float(loss.detach())


def main():
    if not torch.cuda.is_available():
        sys.exit("train_depth.py trains on the GPU; there is none here")
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    steps, runs, precision = opt_arg("--steps", 500, int), opt_arg("--runs", 3, int), opt_arg("--precision", "f16x3", str)
    dev = torch.device("cuda:0")
    pose, K, _ = S.ball_cameras(seed=0, radius=3.0, H=H, W=W)
    pose, K = pose.to(dev), K.to(dev)
    C = pose.shape[0]
    test_ids = list(range(5, C, 22))
    scene = (pose, torch.linalg.inv(K), S.blob_scene_images(pose, K, H, W), S.blob_scene_depth_images(pose, K, H, W),
             [i for i in range(C) if i not in test_ids], test_ids)
    share = float(torch.stack([(scene[3][i] > 0).float().mean() for i in test_ids]).mean())
    lines = [f"depth term on the procedural blob scene {H}x{W}, {N_RAYS} rays x {steps} steps, 64x2 samples, {precision}, RAdam lr 2e-3, one MI355X;",
             f"held-out views {test_ids} ({100 * share:.0f} % of their pixels have a depth target); {runs} seeds per setting",
             "depth_weight  seed   psnr dB   mean |depth - analytic| on the object   opacity on the object   selected share (last 20 steps)   empty   last loss"]
    for lam in (0.0, 0.1, 1.0):
        rows = [run(dev, scene, lam, precision, steps, seed) for seed in range(runs)]
        for seed, (p, e, a, s, l) in enumerate(rows):
            lines.append(f"{lam:12.1f}  {seed:4d}   {p:7.2f}   {e:14.4f}   {a:10.3f}   {s:10.4f}   {'yes' if a < 0.5 else 'no':>5s}   {l:.5f}")
        lines.append(f"{lam:12.1f}  mean   {sum(r[0] for r in rows) / runs:7.2f}   {sum(r[1] for r in rows) / runs:14.4f}   "
                     f"{sum(r[2] for r in rows) / runs:10.3f}   {sum(r[3] for r in rows) / runs:10.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
