"""fp64 restatement of the expected depth and of the composite backward that takes a gradient on it (csrc/depth.hip, the geometry
library), built on composite_ref / mask_ref / distortion_ref (M.variant through D.variant, M.forward64, D.weights64,
D.dist_prefix, O.composite), and the same computation in fp32 torch for the bar.  Not a test module.

    w_j   = the rgb composite's weights (composite_ref: same eps draw, same 1e-10, delta not scaled by |d|, 1e10 for the last sample)
    zexp  = sum_{j <= S-1} w_j z_j,  z_j the rounded fp32 depths (the far-plane sample takes part at its depth)
    d_rz  = d (sum rgb * d_rgb + sum zexp * d_zexp) / d sig_rgb                               (autograd; depths are constants)
    d_z   = d (sum zexp * d_zexp) / d sig_rgb
    d_all = d (sum rgb * d_rgb + sum fg * d_fg + sum dist * d_dist + sum zexp * d_zexp) / d sig_rgb

The distortion term inside d_all is the prefix-sum form, which tests/test_distortion_cpu.py holds to the O(S^2) definition to 1e-12 on
every variant.  The closed form of the new term, per sample (`closed_form`): d zexp / d alpha_j = T_j z_j - sum_{k>j} w_k z_k / u_j.
d_zexp ~ N(0,1) per ray is drawn here.  `loss64` is the training term in fp64, the n_valid = 0 branch included.
"""
import torch
import torch.nn.functional as F

import composite_ref as R
import distortion_ref as D
import mask_ref as M
from oracle import mcnerf_oracle as O

NEAR, FAR = D.NEAR, D.FAR
ALL_FOUR = ("edge_S65", "edge_S129", "lds_S1024")          # the shapes whose backward is also checked with all four gradients


def variant(shape, family, rows, white_back):
    """distortion_ref.variant (mask_ref.variant + d_dist) plus d_zexp [N]; seeded: every call returns the same tensors."""
    inp = D.variant(shape, family, rows, white_back)
    g = torch.Generator().manual_seed(M._base_case(shape, rows)["seed"] + 277)
    inp["d_zexp"] = torch.randn(inp["sig_rgb"].shape[0], generator=g)
    return inp


def _terms64(inp, sr):
    """fp64 (rgb, fg, w, s, z) of a variant on the leaf `sr`: M.forward64's outputs and D.weights64's."""
    rgb, fg = M.forward64(sr, M._z32(inp), inp["eps"], inp["white_back"])
    w, s, z = D.weights64(inp, sr)
    return rgb, fg, w, s, z


def reference(inp, all_four=False):
    """fp64: zexp [N], d_rz and d_z [N,S,4] and, with `all_four`, d_all."""
    sr = inp["sig_rgb"].double().clone().requires_grad_(True)
    rgb, fg, w, s, z = _terms64(inp, sr)
    zexp = (w * z).sum(dim=1)
    t_rgb, t_z = (rgb * inp["d_rgb"].double()).sum(), (zexp * inp["d_zexp"].double()).sum()
    out = {"zexp": zexp.detach(), "d_rz": torch.autograd.grad(t_rgb + t_z, sr, retain_graph=True)[0],
           "d_z": torch.autograd.grad(t_z, sr, retain_graph=True)[0]}
    if all_four:
        total = t_rgb + t_z + (fg * inp["d_fg"].double()).sum() + (D.dist_prefix(w, s) * inp["d_dist"].double()).sum()
        out["d_all"] = torch.autograd.grad(total, sr)[0]
    return out


def restated32(inp, all_four=False):
    """The same outputs in fp32 torch: the oracle's weights (O.composite), fp32 sums and fp32 autograd, on the same rounded depths."""
    sr = inp["sig_rgb"].clone().requires_grad_(True)
    z32 = M._z32(inp)
    rgb, _, _, w = O.composite(sr, inp["rays_d"], z32, inp["eps"], inp["white_back"])
    zexp = (w * z32).sum(dim=1)
    t_rgb, t_z = (rgb * inp["d_rgb"]).sum(), (zexp * inp["d_zexp"]).sum()
    out = {"zexp": zexp.detach(), "d_rz": torch.autograd.grad(t_rgb + t_z, sr, retain_graph=True)[0],
           "d_z": torch.autograd.grad(t_z, sr, retain_graph=True)[0]}
    if all_four:
        fg = w[:, :-1].sum(dim=1)
        total = t_rgb + t_z + (fg * inp["d_fg"]).sum() + (D.dist_prefix(w, (z32 - NEAR) * D.Z_SCALE) * inp["d_dist"]).sum()
        out["d_all"] = torch.autograd.grad(total, sr)[0]
    return out


def alpha_forms(inp):
    """fp64, per sample: (autograd d zexp / d alpha_j with alpha a leaf, the closed form T_j z_j - sum_{k>j} w_k z_k / u_j)."""
    z = M._z32(inp).double()
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], dim=-1)
    alpha = (1.0 - torch.exp(-delta * F.softplus(inp["sig_rgb"][..., 0].double() + inp["eps"].double()))).requires_grad_(True)
    u = 1.0 - alpha + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(u[:, :1]), u], dim=-1), dim=-1)[:, :-1]
    w = alpha * T
    auto = torch.autograd.grad((w * z).sum(), alpha)[0]
    wz = (w * z).detach()
    after = torch.cat([wz[:, 1:], torch.zeros_like(wz[:, :1])], dim=1).flip(1).cumsum(1).flip(1)      # sum_{k>j} w_k z_k (no w_j in it)
    return auto, T.detach() * z - after / u.detach()


def loss64(zexp_c, zexp_f, d_gt, near, far, weight):
    """fp64: (weight * m, m, n_valid, d_c, d_f | None) of the depth term; a target is valid iff it is finite and > 0, n_valid = 0
    gives an exact zero and zero gradients."""
    d = d_gt.double()
    valid = torch.isfinite(d) & (d > 0)
    nv = int(valid.sum())
    zs = 1.0 / (float(far) - float(near))
    d0 = torch.where(valid, d, torch.zeros_like(d))
    grads, m = [], 0.0
    for zx in (zexp_c, zexp_f):
        if zx is None:
            grads.append(None)
            continue
        e = torch.where(valid, (zx.double() - d0) * zs, torch.zeros_like(d))   # s(a) - s(b) = (a - b) z_scale
        m = m + float((e * e).sum()) / max(nv, 1)
        grads.append(2.0 * weight * zs / max(nv, 1) * e)
    return weight * m, m, nv, grads[0], grads[1]
