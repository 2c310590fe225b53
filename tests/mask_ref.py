"""fp64 restatement of the FRONT weight and of the composite backward that takes a gradient on it (csrc/mask.hip, the extension
library), built on composite_ref.make / depths / _weights, and the same computation in fp32 torch (the oracle's
composite, as composite_ref.oracle32) for the bar.  Not a test module.

    w_j  = the rgb composite's weights (composite_ref: same eps draw, same 1e-10, delta not scaled by |d|, 1e10 for the last sample)
    fg   = sum_{j <= S-2} w_j            (the far-plane sample left out: sum_j w_j is 1 on every ray)
    d_sig_rgb = d (sum rgb * d_rgb + sum fg * d_fg) / d sig_rgb        (autograd)

Two input families on the shapes of composite_ref.CASES:
  "a"  the unmodified case: saturated, opaque and empty rays -- every non-planted ray has fg = 1 and the d_fg term gives nothing;
  "b"  its SEMI-TRANSPARENT variant: rays 0-3 are kept, every ray from 4 on is redrawn with its own tau ~ U(0.1, 3),
       sigma_raw = log(expm1(tau / 7)) + 0.3 N(0,1) (optical depth about tau over the depth range of 7) and its eps scaled by 0.3.
       `FRACTION`: in every variant with N = 53 and S >= 3 at least that share of the rays has fg in (0.05, 0.95) (asserted on the
       CPU by tests/test_mask_cpu.py; measured 0.81 - 0.92).
A variant also chooses the depth form (grid / rows) and white_back, whatever the table's case has: `variant(name, family, rows, wb)`.
d_fg ~ N(0,1) per ray is drawn here (the table has none).
"""
import torch

import composite_ref as R
from oracle import mcnerf_oracle as O

FRACTION = 0.7
# the shapes the issue of the feature names: chunk edges, the LDS switch, the bound, one ray, the grid-stride case
SHAPES = ("edge_S2", "edge_S3", "edge_S63", "edge_S64", "edge_S65", "edge_S129", "lds_S1024", "lds_S2048", "one_ray", "stride")
_BASE = {"one_ray": "one_ray", "stride": "stride"}


def _base_case(shape, rows):
    """The table case a shape is drawn from, with the depth form asked for (the planted maxima of "stride" need rows: off on the grid)."""
    name = _BASE.get(shape, f"{shape}_{'rows' if rows else 'grid'}")
    c = dict(R.CASES[name], rows=rows)
    if not rows:
        c["maxima"] = False
    return c


def variant(shape, family, rows, white_back):
    """The inputs of composite_ref.make for one variant, plus d_fg [N]; seeded: every call returns the same tensors."""
    c = dict(_base_case(shape, rows), white_back=white_back)
    key = "\0mask_ref"
    R.CASES[key] = c                        # (composite_ref.make draws by name: a temporary entry, gone before anything else looks)
    try:
        inp = R.make(key)
    finally:
        del R.CASES[key]
    N, S = c["N"], c["S"]
    g = torch.Generator().manual_seed(c["seed"] + 77)
    inp["d_fg"] = torch.randn(N, generator=g)
    if family == "b" and N > 4:
        tau = 0.1 + 2.9 * torch.rand(N - 4, 1, generator=g)
        inp["sig_rgb"][4:, :, 0] = torch.log(torch.expm1(tau / 7.0)) + 0.3 * torch.randn(N - 4, S, generator=g)
        inp["eps"][4:] *= 0.3
    else:
        assert family in ("a", "b")
    return inp


def _z32(inp):
    return R.depths(inp["z"], inp["jitter"], inp["sig_rgb"].shape[0])


def forward64(sig_rgb, z32, eps, white_back):
    """fp64 (rgb [N,3], fg [N]) on the rounded depths; sig_rgb may be an fp64 leaf."""
    sr, z = sig_rgb.double(), z32.double()
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], dim=-1)
    w = R._weights(delta, sr[..., 0] + eps.double())
    rgb = (w.unsqueeze(-1) * sr[..., 1:]).sum(dim=1)
    if white_back:
        rgb = rgb + 1.0 - w.sum(dim=1, keepdim=True)
    return rgb, w[:, :-1].sum(dim=1)


def reference(inp, d_rgb=None):
    """fp64: fg [N] and d_sig_rgb [N,S,4] of sum rgb * d_rgb + sum fg * d_fg (`d_rgb` None: the case's; pass zeros for the d_fg term alone)."""
    sr = inp["sig_rgb"].double().clone().requires_grad_(True)
    rgb, fg = forward64(sr, _z32(inp), inp["eps"], inp["white_back"])
    d_rgb = inp["d_rgb"] if d_rgb is None else d_rgb
    ((rgb * d_rgb.double()).sum() + (fg * inp["d_fg"].double()).sum()).backward()
    return {"fg": fg.detach(), "d_sig_rgb": sr.grad}


def restated32(inp, d_rgb=None):
    """The same two outputs in fp32 torch: the oracle's composite (O.composite) and fp32 autograd, on the same rounded depths."""
    sr = inp["sig_rgb"].clone().requires_grad_(True)
    rgb, _, _, w = O.composite(sr, inp["rays_d"], _z32(inp), inp["eps"], inp["white_back"])
    fg = w[:, :-1].sum(dim=1)
    d_rgb = inp["d_rgb"] if d_rgb is None else d_rgb
    ((rgb * d_rgb).sum() + (fg * inp["d_fg"]).sum()).backward()
    return {"fg": fg.detach(), "d_sig_rgb": sr.grad}


def bound(e_fp32, ref):
    """The bar of a kernel output against fp64: 2 x the fp32 restatement's own error on the case + 16 ulp of the largest reference value
    (the rule of tests/test_multicam_gpu.py: the kernel sums the same fp32 terms in another order)."""
    return 2.0 * e_fp32 + 16.0 * 2.0 ** -24 * float(ref.abs().max())


def semi_transparent_share(fg):
    return float(((fg > 0.05) & (fg < 0.95)).double().mean())
