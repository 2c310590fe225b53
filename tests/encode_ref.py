"""fp64 restatement of the stand-alone positional encoding of csrc/select.hip (encode_kernel / encode_bwd_kernel; SinCosEmbedding of the
reference, oracle.mcnerf_oracle.embed) and the ONE table of cases that tests/test_encode_ref_cpu.py (fp32 torch against this
restatement, no GPU) and tests/test_encode_ops_gpu.py (the kernels against it) both run.  Not a test module.

    out [n, 3 + 6 F] = [x, y, z, per axis c: w_f sin(2^f x_c) f < F, w_f cos(2^f x_c) f < F]
    d_x_c            = g_c + sum_f w_f 2^f (cos(2^f x_c) g_sin(c, f) - sin(2^f x_c) g_cos(c, f)),  abs_sum the same with magnitudes

The argument is formed as the kernel and the reference model both form it: fl32(x * 2^f), which is exact (a power of two).  Sine and
cosine of it are then taken in float64 and multiplied by the fp32 BARF weight, widened.

The bars.  Forward: |err| <= 4 * 2^-24 * w_f per channel; the three pass-through channels are bit-exact, channels with w_f = 0 exactly
0.0.  Why four units: torch's CPU fp32 sin and cos are within 0.6 units of the fp64 value on these inputs, and with the rounding of
the product by a partial weight within 1.44 units of w_f (test_encode_ref_cpu.py measures both and asserts <= 1 and <= 2); the
polynomial of mcn_sincos evaluated step by step in fp32 is within 1.54 units.  Four leaves the reference half the bar and the kernel's own arithmetic a factor of 2.6.
Backward: 8 * 2^-24 * abs_sum; fp32 autograd over the oracle's formulation stays within half of it.

Cases: F x n x BARF weights x the spread of x.  n * 3 F threads run the forward, n * 3 the backward (256 per block): F = 10 puts n = 8, 9
at 240 / 270 threads; n = 85, 86 are 255 / 258 threads of the backward (and of the F = 1 forward).  The planted values take the first
elements of x (as many as fit): signed zeros, 1e-30, +-3.5 (the scene bound), the fp32 neighbours of pi/4, pi/2, 3 pi/4, pi -- quarter-
turn boundaries of the range reduction at the first octave -- and the same divided by 2^9, which land there at the top octave."""
import math

import torch

from oracle import mcnerf_oracle as O

U24 = 2.0 ** -24
# Worst |fp32 torch - fp64| measured on the CPU by test_encode_ref_cpu.py over all cases (never the kernel's):
TOL = {
    "fwd": 4.0,             # units of 2^-24 w_f:      worst 1.44 (a partial weight: the product rounds again; bare sin / cos: 0.60)
    "bwd": 8.0,             # units of 2^-24 abs_sum:  worst 3.65
}
FREQS = (0, 1, 4, 6, 10)
POINTS = (1, 8, 9, 85, 86, 777)
WEIGHTS = ("ones", "mid", "zeros")
SPREADS = (7.0, 200.0)
BARF = dict(barf_start=0.3846, barf_end=0.6923, step_r=0.55)            # the schedule of the mid-ramp weights
_Q = [float(torch.tensor(k * math.pi / 4, dtype=torch.float32)) for k in (1, 2, 3, 4)]
PLANTS = (0.0, -0.0, 1e-30, 3.5, -3.5, *_Q, *(q / 512.0 for q in _Q))
FUSED_CASE = "F10_n777_ones_x7"            # also compared with the encoding the fused MLP forward saves


def _case(F, n, weights, spread, seed):
    return dict(F=F, n=n, weights=weights, spread=spread, seed=seed)


CASES = {}
for _F in FREQS:
    for _n in POINTS:
        for _w in (WEIGHTS if _F else WEIGHTS[:1]):            # (F = 0 has no weights)
            for _s in SPREADS:
                CASES[f"F{_F}_n{_n}_{_w}_x{int(_s)}"] = _case(_F, _n, _w, _s, 10000 * _F + 10 * _n + WEIGHTS.index(_w) + int(_s))


def weights(kind, F):
    """fp32 [F]: all ones; the BARF schedule mid-ramp (ones, one partial weight, exact zeros); ones with the upper half exactly zero."""
    if kind == "ones" or F == 0:
        return torch.ones(F, dtype=torch.float32)
    if kind == "mid":
        return O.barf_weights(BARF["step_r"], O.RenderCfg(n_freqs=F, barf_mode=True, barf_start=BARF["barf_start"], barf_end=BARF["barf_end"]))
    w = torch.ones(F, dtype=torch.float32)
    w[F // 2:] = 0.0
    return w


def make(name):
    """The case's fp32 inputs (host): x [n,3], barf_w [F], d_out [n, 3 + 6 F] ~ N(0,1).  Seeded."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    x = c["spread"] * (torch.rand(c["n"], 3, generator=g) - 0.5)
    k = min(len(PLANTS), x.numel())
    x.view(-1)[:k] = torch.tensor(PLANTS[:k], dtype=torch.float32)
    return dict(x=x, barf_w=weights(c["weights"], c["F"]), d_out=torch.randn(c["n"], 3 + 6 * c["F"], generator=g))


def _sincos(x, F):
    """sin, cos [n,3,F] in fp64 of the fp32 arguments fl32(x * 2^f)."""
    assert x.dtype == torch.float32
    arg = x.unsqueeze(-1) * (2.0 ** torch.arange(F, dtype=torch.float32))
    assert torch.equal(arg.double(), x.double().unsqueeze(-1) * (2.0 ** torch.arange(F, dtype=torch.float64)))       # exact
    return arg.double().sin(), arg.double().cos()


def reference(inp):
    """-> dict(out [n, 3 + 6 F], d_x [n,3], abs_sum = dict(out, d_x)), fp64."""
    x, w, g = inp["x"], inp["barf_w"].double(), inp["d_out"].double()
    n, F = x.shape[0], w.numel()
    s, c = _sincos(x, F)
    out = torch.cat([x.double(), torch.cat([s * w, c * w], dim=-1).reshape(n, 6 * F)], dim=-1)
    gs = g[:, 3:].reshape(n, 3, 2 * F)
    k = w * 2.0 ** torch.arange(F, dtype=torch.float64)
    d_x = g[:, :3] + (k * (c * gs[..., :F] - s * gs[..., F:])).sum(-1)
    mag = g[:, :3].abs() + (k * ((c * gs[..., :F]).abs() + (s * gs[..., F:]).abs())).sum(-1)
    return {"out": out, "d_x": d_x, "abs_sum": {"out": out.abs(), "d_x": mag}}


def embed32(x, w):
    """oracle.mcnerf_oracle.embed in fp32 with the weights given (it is O.embed bit for bit where O.embed can form them)."""
    F = w.numel()
    arg = x.unsqueeze(-1) * (2.0 ** torch.linspace(0, F - 1, F, dtype=torch.float32) if F else torch.zeros(0))
    enc = torch.cat([arg.sin(), arg.cos()], dim=-1) * torch.cat([w, w])
    return torch.cat([x, enc.reshape(x.shape[0], 6 * F)], dim=-1)


def torch32(inp):
    """The same outputs from fp32 torch: embed32 and its fp32 autograd."""
    x = inp["x"].clone().requires_grad_(True)
    out = embed32(x, inp["barf_w"])
    (out * inp["d_out"]).sum().backward()
    return {"out": out.detach(), "d_x": x.grad}


def channel_weights(w):
    """[3 + 6 F] fp64: the weight of every output channel (1 for the pass-through channels)."""
    return torch.cat([torch.ones(3, dtype=torch.float64), torch.cat([w, w]).double().repeat(3)])


def compare(label, got, ref, w, tol_scale=1.0, exact=True):
    """`got` (out and / or d_x) against `ref` under the bars * tol_scale -> ({key: worst error in units of 2^-24 w_f / 2^-24 abs_sum},
    list of failure messages).  exact: the pass-through channels must hold the bits of x."""
    units, bad = {}, []
    if got.get("out") is not None:
        o = got["out"].detach().cpu()
        assert tuple(o.shape) == tuple(ref["out"].shape), (label, tuple(o.shape))
        if o.numel():
            if exact and not torch.equal(o[:, :3].view(torch.int32), ref["out"][:, :3].float().view(torch.int32)):
                bad.append(f"[{label}] out: the pass-through channels are not the bits of x")
            cw = channel_weights(w)
            e = (o.double() - ref["out"]).abs()
            e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
            b = tol_scale * TOL["fwd"] * U24 * cw                                  # (a channel with w_f = 0: exactly 0.0)
            u = torch.where(e == 0, torch.zeros_like(e), e / (U24 * cw).clamp_min(1e-300))
            units["out"] = float(u[:, 3:].max()) if o.shape[1] > 3 else 0.0
            if bool((e[:, 3:] > b[3:]).any()):
                i, j = (int(v) for v in torch.unravel_index((e / b.clamp_min(1e-300))[:, 3:].reshape(-1).argmax(), e[:, 3:].shape))
                bad.append(f"[{label}] out: error {float(e[i, 3 + j]):.3e} > {float(b[3 + j]):.3e} at point {i}, channel {3 + j}: got "
                           f"{float(o[i, 3 + j]):.9g}, reference {float(ref['out'][i, 3 + j]):.9g}")
    if got.get("d_x") is not None:
        d = got["d_x"].detach().cpu().double()
        assert tuple(d.shape) == tuple(ref["d_x"].shape), (label, tuple(d.shape))
        if d.numel():
            e = (d - ref["d_x"]).abs()
            e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
            a = ref["abs_sum"]["d_x"]
            units["d_x"] = float(torch.where(e == 0, torch.zeros_like(e), e / (U24 * a).clamp_min(1e-300)).max())
            b = tol_scale * TOL["bwd"] * U24 * a
            if bool((e > b).any()):
                i, j = (int(v) for v in torch.unravel_index((e / b.clamp_min(1e-300)).reshape(-1).argmax(), e.shape))
                bad.append(f"[{label}] d_x: error {float(e[i, j]):.3e} > {float(b[i, j]):.3e} at point {i}, axis {j}: got {float(d[i, j]):.9g}, "
                           f"reference {float(ref['d_x'][i, j]):.9g}")
    return units, bad


def line(label, units):
    return f"[encode, {label}] error in units of 2^-24: " + "  ".join(f"{k} {v:.2f}" for k, v in units.items())
