"""Convergence experiment of the per-camera colour calibration: does the calibrated loss undo per-camera exposure /
white-balance / black-level differences that would otherwise be baked into the field?

    python scripts/train_color_calib.py [--steps 500] [--runs N] [--lr-color LR] [--beta1-color B] [--reg LAMBDA] [--out profiles/color_calib_convergence.txt] [dense|lazy]

The trailing `lazy` makes the colour group row-lazy (`"lazy_rows": True`): a camera's row steps only when the camera is the
step's; `dense` (the default) is the experiment as it was recorded.

The radiance-field loop is tests/test_y_convergence_gpu._field_run, imported and run as it is (procedural blob scene, 110-camera Ball
rig, 100 x 100 float images, 4096 rays per step, f16x3h, one seed); three runs:
  A  clean images, no calibration (`_field_run` itself);
  B  the training images passed through synthetic.camera_color_response (gain spread 0.15, bias spread 0.03), no calibration;
  C  the images of B, the loss through MC_NeRF_Loss.get_rgb_loss_calibrated with a [C,6] parameter of its own in the optimiser.
The held-out PSNR is what the loop returns: the canonical (uncorrected) render of the held-out cameras against the CLEAN images.
Also reported: the rms error of the recovered relative gains g / mean(g) of the training cameras over that of the identity.
tests/test_color_calib_gpu.py gates the same three runs through `field_run_with`."""
import argparse
import os
import sys
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GAIN_SPREAD, BIAS_SPREAD = 0.15, 0.03
STEPS = 500
PRECISION = "f16x3h"
# The colour group of the loop's RAdam.  weights_color is row-sparse in this loop -- only the step's ONE camera has a gradient, a camera is
# visited ~5 times in 500 steps -- so the group runs WITHOUT momentum (beta1 = 0): with beta1 = 0.9 a row keeps moving on a stale gradient
# for ~10 steps after its camera has left, and is never corrected until the next visit ~100 steps later.  With beta1 = 0 a row moves at a
# visit only, by lr * g / rms(g); the rms runs over all steps, the ~99 % with a zero gradient included, so a typical gradient moves the
# row by ~10 lr: lr = 1e-2 makes that the scale of the gain spread to recover (0.1).  (The loop's own 2e-3 / 0.9 moved the rows a tenth
# of the way: C 19.65-19.81 dB, ratio 0.90, measured four times.  RAdam keeps its step-size cache per group, so this group's step size
# is beta1 = 0's.)
LR_COLOR = 1e-2
BETAS_COLOR = (0.0, 0.999)


def rig_split():
    """(C, train ids, held-out ids) of `_field_run`'s rig."""
    from mc_nerf_amd import synthetic as S
    C = S.ball_cameras(seed=0, radius=3.0, H=100, W=100)[0].shape[0]
    test_ids = list(range(5, C, 22))
    return C, [i for i in range(C) if i not in test_ids], test_ids


def field_run_with(dev, response=None, calibrate=False, seed=0, steps=STEPS, lr_color=LR_COLOR, reg=None, betas_color=BETAS_COLOR, lazy=False):
    """`_field_run(dev, PRECISION, steps, seed)` with the ground truth of every TRAINING step passed through its camera's colour response
    (`response` = (gain, bias) [C,3] on `dev`) and, with `calibrate`, the loss replaced by get_rgb_loss_calibrated on a zero [C,6]
    parameter that joins the loop's optimiser as a second group (`lr_color`, `betas_color`, `lazy`: a row-lazy group; `reg` None: the default "color_calib_reg").  The loop's
    camera of every step is its own host-side draw, repeated here (no device read-back).  -> (held-out PSNR against the clean
    images, the [C,6] parameter | None)."""
    import test_y_convergence_gpu as Y
    import mc_nerf_amd.model as M
    C, train_ids, _ = rig_split()
    order = torch.randint(len(train_ids), (steps,), generator=torch.Generator().manual_seed(seed)).tolist()
    state = {"step": 0, "w": None}
    plain = M.MC_NeRF_Loss.get_rgb_loss

    def rgb_loss(self, rgbs):
        rgb_c, rgb_f, gt = rgbs
        cam = train_ids[order[state["step"]]]
        state["step"] += 1
        if response is not None:
            gt = response[0][cam] * gt + response[1][cam]
        if not calibrate:
            return plain(self, [rgb_c, rgb_f, gt])
        return self.get_rgb_loss_calibrated([rgb_c, rgb_f, gt], state["w"], [cam], [0, rgb_c.shape[0]], reg=reg)

    class RAdamWithColour(M.RAdam):
        def __init__(self, params, **kw):
            state["w"] = torch.nn.Parameter(torch.zeros(C, 6, device=dev))
            group = {"params": [state["w"]], "lr": lr_color}
            if betas_color is not None:
                group["betas"] = tuple(betas_color)
            if lazy:
                group["lazy_rows"] = True
            super().__init__([{"params": list(params)}, group], **kw)

    with mock.patch.object(M.MC_NeRF_Loss, "get_rgb_loss", rgb_loss), mock.patch.object(M, "RAdam", RAdamWithColour if calibrate else M.RAdam):
        psnr, _, _ = Y._field_run(dev, PRECISION, steps, seed=seed)
    assert state["step"] == steps
    return psnr, state["w"]


def experiment(dev, steps=STEPS, lr_color=LR_COLOR, reg=None, seed=0, betas_color=BETAS_COLOR, lazy=False):
    """The three runs -> dict(psnr_a, psnr_b, psnr_c, gain_ratio, text)."""
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd.model.loss import COLOR_CALIB_REG
    C, train_ids, _ = rig_split()
    gain, bias = S.camera_color_response(C, seed=1, gain_spread=GAIN_SPREAD, bias_spread=BIAS_SPREAD)
    response = (gain.to(dev), bias.to(dev))
    psnr_a, _ = field_run_with(dev, seed=seed, steps=steps)
    psnr_b, _ = field_run_with(dev, response, seed=seed, steps=steps)
    psnr_c, w = field_run_with(dev, response, calibrate=True, seed=seed, steps=steps, lr_color=lr_color, reg=reg, betas_color=betas_color, lazy=lazy)
    g_hat, g_true = (1.0 + w.detach()[train_ids, :3]).cpu().double(), gain[train_ids].double()
    rel = lambda g: g / g.mean(0, keepdim=True)
    rms = lambda x: float((x ** 2).mean().sqrt())
    ratio = rms(rel(g_hat) - rel(g_true)) / rms(1.0 - rel(g_true))
    text = (f"procedural scene 100x100, 4096 rays x {steps} steps, {PRECISION}, gain spread {GAIN_SPREAD}, bias spread {BIAS_SPREAD}, "
            f"color_calib_reg {COLOR_CALIB_REG if reg is None else reg:g} (not tuned), colour group lr {lr_color:g} betas {tuple(betas_color)}{' lazy rows' if lazy else ''}: held-out PSNR against the clean "
            f"images A (clean, off) {psnr_a:.2f} dB, B (perturbed, off) {psnr_b:.2f} dB, C (perturbed, on) {psnr_c:.2f} dB; "
            f"rms error of the relative gains / identity's {ratio:.3f}")
    return dict(psnr_a=psnr_a, psnr_b=psnr_b, psnr_c=psnr_c, gain_ratio=ratio, text=text)


def record(lines, path=None):
    """Writes the record (this script alone does; the test prints its line)."""
    path = path or os.path.join(ROOT, "profiles", "color_calib_convergence.txt")
    with open(path, "w") as f:
        f.write("# the colour-calibration convergence experiment: one line per run of scripts/train_color_calib.py (the same seed; runs differ by\n"
                "# the order of the weight-gradient atomics)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--lr-color", type=float, default=LR_COLOR)
    ap.add_argument("--beta1-color", type=float, default=BETAS_COLOR[0])
    ap.add_argument("--reg", type=float, default=None)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("camera_group", nargs="?", choices=["dense", "lazy"], default="dense")
    args = ap.parse_args()
    lines = []
    for run in range(args.runs):
        r = experiment(torch.device("cuda:0"), steps=args.steps, lr_color=args.lr_color, reg=args.reg, betas_color=(args.beta1_color, BETAS_COLOR[1]),
                       lazy=args.camera_group == "lazy")
        lines.append(f"run {run + 1}: " + r["text"])
        print(lines[-1], flush=True)
    record(lines, args.out)
