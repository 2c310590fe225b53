"""The closed-form side of the per-camera radial lens model (`lens_model` = "radial") in plain torch.

lens [C,2] = (k1, k2) per camera, OpenCV's two-coefficient radial model: with (x_u, y_u) the ideal normalised image coordinates
and (x_d, y_d) the observed ones,

    r_u^2 = x_u^2 + y_u^2,   D(r) = 1 + k1 r^2 + k2 r^4,   (x_d, y_d) = D(r_u) (x_u, y_u)

World -> pixel is this closed form (`distort_pixels`: the calibration-tag reprojection, C x 5 points, carried by autograd).
Pixel -> ray needs the inverse; on the train path it is the fixed-count Newton iteration of csrc/mcnerf_lens.h.  `undistort_radius`
here is the same root run to convergence in the caller's dtype: synthetic data generation uses it in fp64.
"""
from __future__ import annotations

import torch

LENS_MODELS = ("pinhole", "radial")


def lens_model_setting(sys_param) -> str:
    """sys_param["lens_model"]: "pinhole" (the default, also an absent key) or "radial"; anything else is a ValueError naming the key."""
    v = sys_param.get("lens_model", "pinhole")
    if not isinstance(v, str) or v not in LENS_MODELS:
        raise ValueError(f"lens_model must be 'pinhole' or 'radial', got {v!r}")
    return v


def distort_pixels(pix: torch.Tensor, K: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """Pinhole pixels pix [..., C, P, 2] of cameras with intrinsics K [C,3,3] -> the pixels a lens with coefficients lens [C,2]
    observes: x = (u - K02) / K00, y = (v - K12) / K11, scaled by D(r), mapped back.  Differentiable in all three inputs; at
    lens = 0 the input's bits come back (the scaled offset is added to `pix`, and that offset is exactly zero)."""
    f, c = K.diagonal(dim1=-2, dim2=-1)[:, None, :2], K[:, None, :2, 2]          # (fx, fy), (cx, cy) as [C,1,2] views
    d = pix - c
    n = d / f
    q = (n * n).sum(-1, keepdim=True)
    lens = lens.to(pix.dtype)
    g = q * (lens[:, None, :1] + lens[:, None, 1:] * q)                            # D - 1
    return torch.addcmul(pix, d, g)


def undistort_radius(rd: torch.Tensor, k1: torch.Tensor, k2: torch.Tensor, steps: int = 60) -> torch.Tensor:
    """The root r of r D(r) = rd by `steps` plain Newton steps from r = rd, in the dtype of `rd` (fp64 for data generation)."""
    r = rd
    for _ in range(steps):
        q = r * r
        r = r - (r * (1.0 + q * (k1 + k2 * q)) - rd) / (1.0 + q * (3.0 * k1 + 5.0 * k2 * q))
    return r


def undistort_normalised(xy: torch.Tensor, lens: torch.Tensor, steps: int = 60) -> torch.Tensor:
    """(x_d, y_d) [..., 2] -> (x_u, y_u): the inverse of the forward model where r D(r) is monotone."""
    rd = xy.norm(dim=-1, keepdim=True)
    r = undistort_radius(rd, lens[..., :1], lens[..., 1:], steps)
    return xy * torch.where(rd > 0, r / torch.where(rd > 0, rd, torch.ones_like(rd)), torch.ones_like(rd))
