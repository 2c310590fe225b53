"""fp64 restatement of the distortion term and of the composite backward that takes a gradient on it (csrc/distortion.hip, the
regulariser library), built on composite_ref / mask_ref (M.variant, M._z32, R._weights, O.composite), and the same
computation in fp32 torch for the bar.  Not a test module.

    w_j  = the rgb composite's weights (composite_ref: same eps draw, same 1e-10, delta not scaled by |d|, 1e10 for the last sample)
    s_j  = (z_j - NEAR) * Z_SCALE,  z_j the rounded fp32 depths, NEAR = 1, FAR = 8 (the range of the tables)
    dist = sum_i sum_j w_i w_j |s_i - s_j|  +  (1/3) sum_{j<S-1} w_j^2 (s_{j+1} - s_j)       (the far sample: no interval term)
    d_full  = d (sum rgb * d_rgb + sum fg * d_fg + sum dist * d_dist) / d sig_rgb            (autograd; depths are constants)
    d_alone = d (sum dist * d_dist) / d sig_rgb

The fp64 reference evaluates the O(S^2) DEFINITION (`dist_pairs`), ray chunk by ray chunk; only the 8453-ray "stride" shape uses the
prefix-sum form (`dist_prefix`), which tests/test_distortion_cpu.py holds to the definition to 1e-12 on every variant (the rows are
non-decreasing there, which it asserts too).  The fp32 restatement: the oracle's weights, the prefix form, fp32 autograd.
d_dist ~ N(0,1) per ray is drawn here.  Z_SCALE is the fp32 rounding of 1/7: the entry points take it as a float.
"""
import torch

import composite_ref as R
import mask_ref as M
from oracle import mcnerf_oracle as O

NEAR, FAR = 1.0, 8.0
Z_SCALE = float(torch.tensor(1.0 / (FAR - NEAR), dtype=torch.float32))
LIVE_DIST, LIVE_SHARE, LIVE_GRAD = 1e-2, 0.7, 1e-3        # the liveness conditions of family "b" (N = 53, S >= 3)
ZERO_TOL = 1e-12                                          # |out| of an identically-zero output: fp64 roundoff of O(1) sums
PAIR_ELEMENTS = 4_000_000                                 # rays x S x S of one chunk of the O(S^2) form


def variant(shape, family, rows, white_back):
    """mask_ref.variant plus d_dist [N]; seeded: every call returns the same tensors."""
    inp = M.variant(shape, family, rows, white_back)
    N = inp["sig_rgb"].shape[0]
    g = torch.Generator().manual_seed(M._base_case(shape, rows)["seed"] + 177)
    inp["d_dist"] = torch.randn(N, generator=g)
    return inp


def is_identically_zero(shape, rows):
    """The S = 2 rows: the one duplicated depth per ray is the only interval, so both samples sit at one depth."""
    return shape == "edge_S2" and rows


def excl_cumsum(x):
    return torch.cat([torch.zeros_like(x[:, :1]), torch.cumsum(x, dim=1)[:, :-1]], dim=1)


def interval_term(w, s, last=None):
    """(1/3) sum_{j<S-1} w_j^2 (s_{j+1} - s_j); `last`: an interval to give the far sample as well (None: it has none)."""
    t = (w[:, :-1] ** 2 * (s[:, 1:] - s[:, :-1])).sum(dim=1)
    if last is not None:
        t = t + w[:, -1] ** 2 * last
    return t / 3.0


def dist_pairs(w, s):
    """The definition, O(S^2) per ray."""
    pair = (w.unsqueeze(2) * w.unsqueeze(1) * (s.unsqueeze(2) - s.unsqueeze(1)).abs()).sum(dim=(1, 2))
    return pair + interval_term(w, s)


def dist_prefix(w, s):
    """The O(S) form of the kernels: equal to the definition on non-decreasing rows."""
    A, B = excl_cumsum(w), excl_cumsum(w * s)
    return 2.0 * (w * (s * A - B)).sum(dim=1) + interval_term(w, s)


def weights64(inp, sig_rgb=None):
    """fp64 (w [N,S], s [N,S], rounded depths) of a variant; `sig_rgb`: an fp64 leaf in place of the variant's."""
    sr = inp["sig_rgb"].double() if sig_rgb is None else sig_rgb
    z = M._z32(inp).double()
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], dim=-1)
    return R._weights(delta, sr[..., 0] + inp["eps"].double()), (z - NEAR) * Z_SCALE, z


def _slice(inp, lo, hi):
    out = {}
    for k, v in inp.items():
        out[k] = v[lo:hi] if isinstance(v, torch.Tensor) and not (k == "z" and v.dim() == 1) else v
    return out


def _chunks(N, S, prefix):
    step = N if prefix else max(1, PAIR_ELEMENTS // (S * S))
    return [(lo, min(N, lo + step)) for lo in range(0, N, step)]


def reference(inp, prefix=False):
    """fp64: dist [N], d_full and d_alone [N,S,4].  `prefix`: the O(S) form (the "stride" shape only)."""
    N, S = inp["sig_rgb"].shape[:2]
    dist, full, alone = [], [], []
    for lo, hi in _chunks(N, S, prefix):
        c = _slice(inp, lo, hi)
        sr = c["sig_rgb"].double().clone().requires_grad_(True)
        w, s, _ = weights64(c, sr)
        rgb = (w.unsqueeze(-1) * sr[..., 1:]).sum(dim=1)
        if c["white_back"]:
            rgb = rgb + 1.0 - w.sum(dim=1, keepdim=True)
        fg = w[:, :-1].sum(dim=1)
        d = dist_prefix(w, s) if prefix else dist_pairs(w, s)
        term = (d * c["d_dist"].double()).sum()
        total = (rgb * c["d_rgb"].double()).sum() + (fg * c["d_fg"].double()).sum() + term
        full.append(torch.autograd.grad(total, sr, retain_graph=True)[0])
        alone.append(torch.autograd.grad(term, sr)[0])
        dist.append(d.detach())
    return {"dist": torch.cat(dist), "d_full": torch.cat(full), "d_alone": torch.cat(alone)}


def restated32(inp):
    """The same three outputs in fp32 torch: the oracle's weights (O.composite), the prefix form and fp32 autograd, same rounded depths."""
    sr = inp["sig_rgb"].clone().requires_grad_(True)
    z32 = M._z32(inp)
    rgb, _, _, w = O.composite(sr, inp["rays_d"], z32, inp["eps"], inp["white_back"])
    fg = w[:, :-1].sum(dim=1)
    d = dist_prefix(w, (z32 - NEAR) * Z_SCALE)
    term = (d * inp["d_dist"]).sum()
    total = (rgb * inp["d_rgb"]).sum() + (fg * inp["d_fg"]).sum() + term
    full = torch.autograd.grad(total, sr, retain_graph=True)[0]
    alone = torch.autograd.grad(term, sr)[0]
    return {"dist": d.detach(), "d_full": full, "d_alone": alone}


def live_share(dist):
    return float((dist > LIVE_DIST).double().mean())
