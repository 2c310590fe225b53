"""Convergence experiment of the per-camera radial lens model: does learning (k1, k2) per training camera undo lens
distortion that a pinhole ray model would otherwise push into the field?

    python scripts/train_lens.py [--steps 500] [--runs 3] [--lr-lens LR] [--beta1-lens B] [--out profiles/lens_convergence.txt]

The radiance-field loop is tests/test_y_convergence_gpu._field_run, imported and run as it is, as scripts/train_color_calib.py does
(procedural blob scene, 110-camera Ball rig with the truth's pose and K, 100 x 100 float images, 4096 rays per step, f16x3h);
four configurations:
  A  clean rig, pinhole rays (`_field_run` itself);
  B  the training images rendered through synthetic.lens_distortion (k1 spread 0.05, k2 spread 0.005), pinhole rays;
  C  the images of B, the rays through RayBatchFn with a zero [C,2] parameter of its own in the optimiser, in a GROUP OF ITS OWN
     (lr, betas below: the parameter is row-sparse, as weights_color is -- only the step's camera has a gradient);
  D  as C with the parameter in the loop's single default group (its lr 2e-3, betas (0.9, 0.999)), for comparison.
The held-out PSNR is what the loop returns: the pinhole render of the held-out cameras (they have no lens parameter) against their
CLEAN images.  Also reported: the rms error of the recovered k1 of the training cameras beside the rms of the true k1 (what a model
that stays at zero scores).  No target is set for either figure."""
import argparse
import os
import sys
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

K1_SPREAD, K2_SPREAD = 0.05, 0.005
STEPS = 500
PRECISION = "f16x3h"
# starting values, NOT tuned: without momentum a row moves at its camera's visits only (train_color_calib.py has the reasoning), by
# ~10 lr per visit at a ~1 % visit rate, ~5 visits per camera in 500 steps; 2e-3 makes that the scale of the k1 spread
LR_LENS = 2e-3
BETAS_LENS = (0.0, 0.999)


def rig():
    from mc_nerf_amd import synthetic as S
    pose, K, _ = S.ball_cameras(seed=0, radius=3.0, H=100, W=100)
    C = pose.shape[0]
    test_ids = list(range(5, C, 22))
    return pose, K, [i for i in range(C) if i not in test_ids], test_ids


def field_run_with(dev, lens_true=None, learn=False, own_group=True, seed=0, steps=STEPS, lr_lens=LR_LENS, betas_lens=BETAS_LENS):
    """`_field_run(dev, PRECISION, steps, seed)` with the TRAINING cameras' images rendered through `lens_true` [C,2] (the held-out
    ones stay clean) and, with `learn`, the training rays through RayBatchFn on a zero [C,2] parameter that joins the loop's
    optimiser (`own_group`: as a second group with `lr_lens`, `betas_lens`; otherwise inside the loop's one group).  The loop's camera
    of every step is its own host-side draw, repeated here.  -> (held-out PSNR against the clean images, the parameter | None)."""
    import test_y_convergence_gpu as Y
    import mc_nerf_amd.model as M
    from mc_nerf_amd import ops, synthetic as S
    from mc_nerf_amd.model.render import RayBatchFn
    pose, K, train_ids, test_ids = rig()
    C, H, W = pose.shape[0], Y.H, Y.W
    order = torch.randint(len(train_ids), (steps,), generator=torch.Generator().manual_seed(seed)).tolist()
    pose_d, kinv_d = pose.to(dev).contiguous(), torch.linalg.inv(K.to(dev)).contiguous()
    state = {"step": 0, "w": None}
    plain_images, plain_raygen = S.blob_scene_images, ops.raygen_fwd

    def images(pose_, K_, H_, W_, chunk=8192):
        state["rendering"] = True                           # (the scene's own pinhole rays are not training rays)
        clean = plain_images(pose_, K_, H_, W_, chunk)
        if lens_true is not None:
            clean[train_ids] = plain_images(pose_[train_ids], K_[train_ids], H_, W_, chunk, lens=lens_true[train_ids])
        state["rendering"] = False
        return clean

    def raygen(pose_i, kinv_i, pix, W_):
        if not learn or state.get("rendering") or state["step"] >= steps:      # (the held-out renders after the loop stay pinhole)
            return plain_raygen(pose_i, kinv_i, pix, W_)
        cam = train_ids[order[state["step"]]]
        state["step"] += 1
        _, d, o, _ = RayBatchFn.apply(pose_d, kinv_d, [cam], [0, int(pix.shape[0])], H, W, None, pix, None, state["w"])
        return d, o

    class RAdamWithLens(M.RAdam):
        def __init__(self, params, **kw):
            state["w"] = torch.nn.Parameter(torch.zeros(C, 2, device=dev))
            if own_group:
                super().__init__([{"params": list(params)}, {"params": [state["w"]], "lr": lr_lens, "betas": tuple(betas_lens)}], **kw)
            else:
                super().__init__(list(params) + [state["w"]], **kw)

    with mock.patch.object(S, "blob_scene_images", images), mock.patch.object(ops, "raygen_fwd", raygen), \
            mock.patch.object(M, "RAdam", RAdamWithLens if learn else M.RAdam):
        psnr, _, _ = Y._field_run(dev, PRECISION, steps, seed=seed)
    assert not learn or state["step"] == steps
    return psnr, state["w"]


def experiment(dev, steps=STEPS, lr_lens=LR_LENS, betas_lens=BETAS_LENS, seed=0):
    """The four configurations -> dict(psnr_a .. psnr_d, k1_rms_c, k1_rms_d, k1_rms_true, text)."""
    from mc_nerf_amd import synthetic as S
    pose, K, train_ids, _ = rig()
    lens = S.lens_distortion(pose.shape[0], seed=1, k1_spread=K1_SPREAD, k2_spread=K2_SPREAD)
    rms = lambda x: float((x.double() ** 2).mean().sqrt())
    psnr_a, _ = field_run_with(dev, seed=seed, steps=steps)
    psnr_b, _ = field_run_with(dev, lens, seed=seed, steps=steps)
    psnr_c, wc = field_run_with(dev, lens, learn=True, seed=seed, steps=steps, lr_lens=lr_lens, betas_lens=betas_lens)
    psnr_d, wd = field_run_with(dev, lens, learn=True, own_group=False, seed=seed, steps=steps)
    err = lambda w: rms(w.detach().cpu()[train_ids, 0] - lens[train_ids, 0])
    out = dict(psnr_a=psnr_a, psnr_b=psnr_b, psnr_c=psnr_c, psnr_d=psnr_d, k1_rms_c=err(wc), k1_rms_d=err(wd), k1_rms_true=rms(lens[train_ids, 0]))
    out["text"] = (f"procedural scene 100x100, 4096 rays x {steps} steps, {PRECISION}, k1 spread {K1_SPREAD}, k2 spread {K2_SPREAD}: held-out PSNR "
                   f"against the clean images A (clean rig, off) {psnr_a:.2f} dB, B (distorted, off) {psnr_b:.2f} dB, C (distorted, on, own group "
                   f"lr {lr_lens:g} betas {tuple(betas_lens)}) {psnr_c:.2f} dB, D (distorted, on, the default single group) {psnr_d:.2f} dB; rms error of "
                   f"the recovered k1 C {out['k1_rms_c']:.4f}, D {out['k1_rms_d']:.4f}, of k1 = 0 {out['k1_rms_true']:.4f}")
    return out


def record(lines, path=None):
    path = path or os.path.join(ROOT, "profiles", "lens_convergence.txt")
    with open(path, "w") as f:
        f.write("# the lens-distortion convergence experiment: one line per run of scripts/train_lens.py (the same seed; runs differ by the\n"
                "# order of the weight-gradient atomics); no target is set, the group's lr / betas are starting values, not tuned\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--lr-lens", type=float, default=LR_LENS)
    ap.add_argument("--beta1-lens", type=float, default=BETAS_LENS[0])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for run in range(args.runs):
        r = experiment(torch.device("cuda:0"), steps=args.steps, lr_lens=args.lr_lens, betas_lens=(args.beta1_lens, BETAS_LENS[1]))
        lines.append(f"run {run + 1}: " + r["text"])
        print(lines[-1], flush=True)
    record(lines, args.out)
