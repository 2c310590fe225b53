"""fp64 restatement of the alpha compositing of csrc/composite.hip (the formulas of oracle.mcnerf_oracle.composite / sigma2weights /
deltas_of, evaluated in float64), and the ONE table of cases that tests/test_composite_ref_cpu.py (fp32 oracle against this
restatement, no GPU) and tests/test_composite_gpu.py (the kernels against it) both run.  Not a test module.

The depth contract.  The kernels form z = fl32(zrow[j] + jitter[n]) with one fp32 rounding and delta = fl32(z[j+1] - z[j]), 1e10 for
the last sample.  The restatement takes the depths ALREADY rounded that way (`depths`: the fp32 sum, then .double()) -- the difference
of two neighbouring depths cancels most of their digits, so depths formed in fp64 would differ from the kernels' by far more than
anything else in the computation.  Everything after that is fp64 (the difference of two fp32 numbers is exact in fp64; its fp32
rounding, where it has one, is a relative 6e-8 of a delta).

    alpha_j = 1 - exp(-delta_j softplus(sigma_j + eps_j)),  u_j = 1 - alpha_j + 1e-10,  w_j = alpha_j prod_{k<j} u_k
    rgb     = sum_j w_j c_j  (+ 1 - sum_j w_j with white_back)
    w_sel   = the same weights with the draw eps_sel
    sd_j    = softplus(sigma_j) delta_j |d|,  p_j = exp(-sum_{k<j} sd_k) (1 - exp(-sd_j)),  opacity = sum_j p_j,  depth = sum_j z_j p_j
    d_sig_rgb = d sum(rgb * d_rgb) / d sig_rgb     (fp64 autograd)

Inputs of a case (`make`): sigma_raw ~ 3 N(0,1), rgb ~ U(0,1), rays_d of length 0.5 .. 1.5, jitter ~ U(0, 0.1), d_rgb ~ N(0,1); depths
either the grid linspace(1, 8, S) or rows of sorted 1 + 7 U(0,1) with one duplicated depth per ray (delta = 0).  Planted rays, from
ray `plant_at` on (N >= 16: 4 + 4 + 2 + 1 of them in this order; smaller N: one each in the order last / empty / opaque / saturated,
as many as fit):
    empty      sigma = -20 throughout (all the weight on the last sample, where delta = 1e10);
    opaque     sigma = +12 on the first half;
    saturated  sigma = 30 throughout: the x > 20 branch of softplus, u = 1e-10 where delta is large, the transmittance underflows;
    last       the LAST sample has sigma = -23: softplus * 1e10 is about 1 there, its alpha far from both 0 and 1.
"""
import torch
import torch.nn.functional as F

from oracle import mcnerf_oracle as O

OUTPUTS = ("rgb", "depth", "opacity", "w_sel", "d_sig_rgb")
# absolute max error of the kernels against this restatement: the bars of test_a_ops_gpu.py::test_composite_fwd_bwd
TOL = {"rgb": 2e-6, "depth": 2e-5, "opacity": 2e-6, "w_sel": 2e-6, "d_sig_rgb": 5e-6}

GRID_WAVES = 8192                   # 2048 blocks x 4 waves (MCN_COMPOSITE_BLOCKS): wave w takes rays w, w + 8192, ...
N_STRIDE = GRID_WAVES + 261
W_PLANT, G_PLANT = GRID_WAVES + 100, GRID_WAVES + 200          # rays of the planted maxima of the grid-stride case


def _case(N, S, rows, white_back=True, jitter=True, seed=0, plant_at=0, maxima=False):
    return dict(N=N, S=S, rows=rows, white_back=white_back, jitter=jitter, seed=seed, plant_at=plant_at, maxima=maxima)


CASES = {}
# chunk edges of the 64-lane walk over the samples, both depth forms
for _S in (2, 3, 63, 64, 65, 127, 129, 160):
    for _rows in (False, True):
        CASES[f"edge_S{_S}_{'rows' if _rows else 'grid'}"] = _case(53, _S, _rows, seed=1000 + 2 * _S + _rows)
# the flag matrix: the two flags that change values (the other two, eps_sel and want_depth, only switch outputs off).  ONE seed: the
# four cases differ in nothing but the flags
for _wb in (True, False):
    for _jit in (True, False):
        CASES[f"flags_wb{int(_wb)}_jit{int(_jit)}"] = _case(53, 65, True, white_back=_wb, jitter=_jit, seed=2000)
# more rays than waves in the grid: every wave of blocks 0 .. 65 walks two rays; the planted rays and both maxima sit in the second
CASES["stride"] = _case(N_STRIDE, 65, True, white_back=False, seed=3000, plant_at=GRID_WAVES + 16, maxima=True)
# the backward's LDS sizes (4 waves x 5 floats per sample): 51 200 B, 81 920 B (the pdf sampler's largest Sc + I), 163 840 B (the bound)
for _N, _S in ((53, 640), (53, 1024), (5, 2048)):
    for _rows in (False, True):
        CASES[f"lds_S{_S}_{'rows' if _rows else 'grid'}"] = _case(_N, _S, _rows, seed=4000 + 2 * _S + _rows)
# (the draw of lds_S2048_grid was changed once, from seed 8096, under the rule of test_composite_ref_cpu.py: there the opaque ray has
#  |d| = 0.61.  On the uniform grid every sample of that ray has the SAME sd = softplus(12) delta |d| = 0.025, so the fp32 rounding of
#  1 - exp(-sd) has the same sign in each of the ~ 1 / sd samples that carry weight and adds up: the fp32 oracle itself was 1.01e-6 off
#  in opacity, past half the bar.  With this draw |d| = 1.31 and the oracle is 3.6e-7 off.)
CASES["lds_S2048_grid"]["seed"] = 8097
CASES["one_ray"] = _case(1, 65, True, seed=5000)


def make(name):
    """The case's fp32 inputs (host): sig_rgb [N,S,4], rays_d [N,3], z ([S] grid or [N,S] rows), jitter [N] | None, eps, eps_sel [N,S],
    d_rgb [N,3], white_back.  Seeded: every call returns the same tensors."""
    c = CASES[name]
    N, S = c["N"], c["S"]
    g = torch.Generator().manual_seed(c["seed"])
    sig_rgb = torch.cat([torch.randn(N, S, 1, generator=g) * 3.0, torch.rand(N, S, 3, generator=g)], -1)
    d = F.normalize(torch.randn(N, 3, generator=g), dim=-1) * (0.5 + torch.rand(N, 1, generator=g))
    jit = torch.rand(N, generator=g) * 0.1
    eps, eps_sel = torch.randn(N, S, generator=g), torch.randn(N, S, generator=g)
    d_rgb = torch.randn(N, 3, generator=g)
    zr = (1.0 + 7.0 * torch.rand(N, S, generator=g)).sort(dim=1).values
    dup = torch.randint(0, S - 1, (N,), generator=g)
    zr[torch.arange(N), dup + 1] = zr[torch.arange(N), dup]              # one duplicated depth per ray: delta = 0
    z = zr if c["rows"] else torch.linspace(1, 8, S)
    # planted rays
    p = c["plant_at"]
    kinds = ["empty"] * 4 + ["opaque"] * 4 + ["saturated"] * 2 + ["last"] if N - p >= 16 else ["last", "empty", "opaque", "saturated"][:N - p]
    for i, kind in enumerate(kinds):
        if kind == "empty":
            sig_rgb[p + i, :, 0] = -20.0
        elif kind == "opaque":
            sig_rgb[p + i, : S // 2, 0] = 12.0
        elif kind == "saturated":
            sig_rgb[p + i, :, 0] = 30.0
        else:
            sig_rgb[p + i, -1, 0] = -23.0
    if c["maxima"]:
        assert c["rows"] and N > G_PLANT
        tail = (4.0 + 4.0 * torch.rand(2, S - 1, generator=g)).sort(dim=1).values
        # the largest selection weight: first sample opaque over a gap of at least 3 -> w_sel = 1 (rays before 8192 stay below 1)
        z[W_PLANT, 0], z[W_PLANT, 1:] = 1.0, tail[0]
        sig_rgb[W_PLANT, :, 0], sig_rgb[W_PLANT, 0, 0], eps_sel[W_PLANT, 0] = -20.0, 30.0, 0.0
        # the largest gradient, in the SIGMA component: first sample softplus(0) = ln 2 over a gap of 1 (alpha = 1/2, d sigma = 1/4 of
        # the white sample's dw = 3 * 8: 6 against the 4 of its colour components), nothing behind it but the last sample, which is black
        z[G_PLANT, 0], z[G_PLANT, 1], z[G_PLANT, 2:] = 1.0, 2.0, tail[1, 1:]
        sig_rgb[G_PLANT, :, 0], sig_rgb[G_PLANT, 0, 0], eps[G_PLANT, 0] = -20.0, 0.0, 0.0
        sig_rgb[G_PLANT, 0, 1:], sig_rgb[G_PLANT, -1, 1:] = 1.0, 0.0
        d_rgb[G_PLANT] = 8.0
    return dict(sig_rgb=sig_rgb.contiguous(), rays_d=d.contiguous(), z=z.contiguous(), jitter=jit if c["jitter"] else None, eps=eps,
                eps_sel=eps_sel, d_rgb=d_rgb, white_back=c["white_back"])


def depths(z, jitter, n_rays):
    """fp32 [N,S]: the kernels' sample depths fl32(z + jitter) of the grid ([S]) or the rows ([N,S]); jitter [N] or None."""
    zr = z.unsqueeze(0).expand(n_rays, -1) if z.dim() == 1 else z
    assert zr.dtype == torch.float32
    return (zr + jitter.reshape(-1, 1)).contiguous() if jitter is not None else zr.contiguous()


def _weights(delta, x):
    alpha = 1.0 - torch.exp(-delta * F.softplus(x))
    u = torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], dim=-1)
    return alpha * torch.cumprod(u, dim=-1)[:, :-1]


def forward(sig_rgb, rays_d, z32, eps, eps_sel, white_back):
    """fp64 forward on the rounded depths z32 (fp32 [N,S]); sig_rgb may be an fp64 leaf -> dict(rgb, depth, opacity, w_sel)."""
    assert z32.dtype == torch.float32
    sr, z = sig_rgb.double(), z32.double()
    sigma, c = sr[..., 0], sr[..., 1:]
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], dim=-1)
    w = _weights(delta, sigma + eps.double())
    rgb = (w.unsqueeze(-1) * c).sum(dim=1)
    if white_back:
        rgb = rgb + 1.0 - w.sum(dim=1, keepdim=True)
    sd = F.softplus(sigma) * (delta * rays_d.double().norm(dim=-1, keepdim=True))
    T = torch.exp(-torch.cat([torch.zeros_like(sd[:, :1]), sd[:, :-1]], dim=1).cumsum(dim=1))
    p = T * (1.0 - torch.exp(-sd))
    return {"rgb": rgb, "depth": (z * p).sum(dim=1, keepdim=True), "opacity": p.sum(dim=1, keepdim=True),
            "w_sel": _weights(delta, sigma + eps_sel.double())}


def reference(inp):
    """Every output of both kernels for the inputs of `make`, fp64: rgb [N,3], depth, opacity [N,1], w_sel [N,S], d_sig_rgb [N,S,4]."""
    sr = inp["sig_rgb"].double().clone().requires_grad_(True)
    z32 = depths(inp["z"], inp["jitter"], inp["rays_d"].shape[0])
    out = forward(sr, inp["rays_d"], z32, inp["eps"], inp["eps_sel"], inp["white_back"])
    (out["rgb"] * inp["d_rgb"].double()).sum().backward()
    out = {k: v.detach() for k, v in out.items()}
    out["d_sig_rgb"] = sr.grad
    return out


def oracle32(inp):
    """The same outputs from the fp32 oracle (O.composite, O.sigma2weights, fp32 autograd) on the same rounded depths."""
    sr = inp["sig_rgb"].clone().requires_grad_(True)
    z32 = depths(inp["z"], inp["jitter"], inp["rays_d"].shape[0])
    rgb, depth, opac, _ = O.composite(sr, inp["rays_d"], z32, inp["eps"], inp["white_back"])
    w_sel = O.sigma2weights(O.deltas_of(z32), inp["sig_rgb"][..., 0], inp["eps_sel"])
    (rgb * inp["d_rgb"]).sum().backward()
    return {"rgb": rgb.detach(), "depth": depth.detach(), "opacity": opac.detach(), "w_sel": w_sel, "d_sig_rgb": sr.grad}


def worst(got, ref):
    """(max |got - ref|, index tuple of it) in fp64; the first index is the ray, the second (w_sel, d_sig_rgb) the sample."""
    e = (got.detach().cpu().double() - ref.detach().cpu().double()).abs()
    if e.numel() == 0:
        return 0.0, ()
    if not bool(torch.isfinite(e).all()):
        e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    k = int(e.reshape(-1).argmax())
    return float(e.reshape(-1)[k]), tuple(int(i) for i in torch.unravel_index(torch.tensor(k), e.shape))


def compare(label, got, ref, tol_scale=1.0):
    """Compares every output present (not None) in `got` with `ref` at TOL * tol_scale -> ({output: max error}, list of failure
    messages naming the output and the ray / sample of the worst error)."""
    errs, bad = {}, []
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        assert tuple(got[k].shape) == tuple(ref[k].shape), (label, k, tuple(got[k].shape), tuple(ref[k].shape))
        e, at = worst(got[k], ref[k])
        errs[k] = e
        if not e <= TOL[k] * tol_scale:
            where = f"ray {at[0]}" + (f", sample {at[1]}" if k in ("w_sel", "d_sig_rgb") else "") + (f", component {at[-1]}" if k in ("rgb", "d_sig_rgb") else "")
            bad.append(f"[{label}] {k}: max error {e:.3e} > {TOL[k] * tol_scale:.1e} at {where}: got {float(got[k][at]):.9g}, reference {float(ref[k][at]):.9g}")
    return errs, bad


def line(label, errs):
    return f"[composite, {label}] " + "  ".join(f"{k} {errs[k]:.2e}" for k in OUTPUTS if k in errs)
