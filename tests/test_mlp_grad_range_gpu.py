"""The backward chains and weight-gradient kernels over the dynamic range of the upstream gradient.

The four reduced-precision modes ("f16x3", "f16x3h", "f16", "bf16") store every dY plane in 16 bits at a per-launch scale
SG = mcn16_grad_scale(word) (csrc/mcnerf_16.h), `word` being the device word composite_bwd leaves: max|d_sig_rgb| of the launch.  The other
op-level tests feed d_out = randn or randn * 1e-4 and never move SG off two values.  Here d_out = g0 * 2^k with max|g0| = 1.5 exactly (so
that word * 2^k is never a power of two by accident; the maximum sits in column 0, where `recover_scale` reads SG back), on the list of
tests/test_mlp_edges_gpu.py (N = 29, S = 40, about 700 listed rows, widths 64 and 256: 8- and 4-wave passes, split and merged skip
segment), "f32" beside the four as the control that has no scale and ignores the word.

References, computed once per width at k = 0 and scaled by 2^k in fp64 (every gradient is linear in d_out):
  * fp64 autograd of the CPU oracle on the kernels' fp32 sample positions, for d_o, d_d and every parameter gradient (f16 / bf16: with
    the kernel's own ReLU decisions, tests/test_mlp16_gpu.py::masked_forward);
  * the fp64 GEMM of the very operands the weight-gradient kernel read, decoded with the RESTATED scale (tests/mlp_edges_ref.py);
  * the scale itself, recovered from the stored dsh plane (`E.recover_scale`) and compared with the restatement `E.grad_scale`: a
    kernel whose SG differs from the documented one fails here even where backward and weight gradient agree with each other.

Gates, all relative to max|ref| at that k (`gates`): ray gradients 1e-3 (f32 / f16x3 / f16x3h, tests/test_mlp_edges_gpu.py) or TOL_GRAD (f16 /
bf16); dW against its own operands 2e-5 max|ref| + 1e-9 * 2^k; dW against autograd: the gates of test_x3_fwd_bwd_indexed (2e-5),
test_x3h_fwd_bwd_dw_indexed (1e-3 of the tensor's largest entry or 5e-7 of the net's) and test_mlp16_fwd_bwd_indexed (TOL_GRAD) without
their max(1, .) floors.  One floor stays, with its reason: at 2e-5 (f32 / f16x3) a BIAS gradient is gated relative to the larger of its
own and its layer's weight gradient's maximum, as tests/test_model_gpu.py::test_sh_degree_topology_matches_reference does: a bias gradient
is a plain signed sum over the rows (sigma.2's is one number), fp32 accumulation errs relative to the summands, not to what is left after
they cancel.  And in f16x3 the floor 5e-7 of the NET's largest gradient that test_x3h_fwd_bwd_dw_indexed already grants f16x3h stays beside
the 2e-5: the planes hold dY * SG in f16 (hi + lo), whose spacing below 2^-14 is 2^-24 whatever the value, so every stored dY entry
carries an absolute error of up to 2^-25 / SG, about 2^-28 of the WORD, however small the entry.  A weight gradient sums `rows` of
them times |X| (694 rows, |X| <= 4: at worst 1e-5 of the word, 5e-7 of the net's largest gradient is 5e-6 of it), so a trunk layer
whose gradient is 1e-4 of the heads' (layers 1 .. 4 here) cannot be held to 2e-5 of its OWN maximum: measured 2e-4 .. 2e-3 of it in
f16x3 against 1e-6 in f32, at every k alike.  The max(1, .) floor of test_x3_fwd_bwd_indexed hid exactly this.

What follows from fp32 itself, not from the kernels, and is therefore not gated (each decided from the fp64 reference, never from the
kernel's output):
  * an entry of the scaled reference that is subnormal in fp32 (0 < |ref| < 2^-126) or beyond FLT_MAX is excluded from the relative
    check: there the kernel must give a subnormal-or-zero, respectively an inf, of the right sign, or anything within the gate.  At
    every |k| <= 100 at most 1 % of a tensor's entries, and none of its 10 largest, may be excluded (asserted);
  * k = -140 and -126: d_out itself is subnormal or borderline.  Every output must be finite; parity is printed, not gated.  The scale
    is 2^100 there (the clamp, `fminf(..., 100.f)`), and the largest stored value 1.5 * 2^(k + 100) <= 1.5 * 2^-26 is below half the
    smallest f16 subnormal: the f16 planes of f16x3 / f16x3h / f16 hold zeros and SG cannot be read from them (`sg_readable`); in bf16
    (8 exponent bits) it is read and must be 2^100.
  * the dy plane identity of (b) in f32 is `dy(k) == dy(0) * 2^k` bit for bit: the f32 kernels have no scale, only linearity.
  * (e), "no other ray is touched": a ray's d_o / d_d is a sum of float atomics, one per 32-row tile (chains: `atomicAdd` after the
    segmented scan of mlp16_bwd.hip / mlp_x3_bwd.hip) or per row tile of the f32 kernel (mlp_bwd.hip: "6 atomics per tile").  Two
    addends commute, three need not: rays whose listed rows lie in at most two such tiles are compared bit for bit, the others at the
    1e-6 max|.| the suite grants the order of lane atomics (tests/test_mlpx3h_gpu.py).
  * the model-level test in f32 is gated at 2e-5 of a tensor's maximum instead of bit for bit, for the same reason: mlp_dw.hip adds every
    workgroup's block with float atomics ("accumulators -> global (float atomics ...)"), so two runs of the same step differ in the last
    bits whatever the loss scale.  Whether the bits were equal is printed.

Run with -s for the measured figures (profiles/mlp_grad_range.txt).
"""
import math
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mlp_edges_ref as E
from oracle import mcnerf_oracle as O
from test_mlp16_gpu import TOL_GRAD, masked_forward
from test_mlpx3h_gpu import assert_planes_match, indexed_case, run_chain

pytestmark = pytest.mark.gpu

WIDTHS = (64, 256)
N_RAYS, N_SAMPLES = 29, 40
SWEEP = (-140, -126, -100, -97, -96, -95, -64, -20, 0, 20, 64, 100, 120)
UNGATED = (-140, -126)                      # the word itself is subnormal or borderline: finite outputs, parity printed
PLANE_KS = (-64, -20, 20, 64)
OVERSTATED = (1, 8, 20)
FLT_MIN, FLT_MAX = 2.0 ** -126, float(np.finfo(np.float32).max)
CHAINS16 = ("f16", "bf16")
PARAMS = [(w, m) for w in WIDTHS for m in E.ALL_MODES]
IDS = [f"{m}-W{w}" for w, m in PARAMS]


def _ops():
    from mc_nerf_amd import ops
    return ops


def word_of(value, dev):
    """The device word composite_bwd leaves for the backward: the fp32 bits of `value`."""
    return torch.tensor([value], dtype=torch.float32, device=dev).view(torch.int32)


@lru_cache(maxsize=None)
def case(width, dev):
    """The list, the net and the base gradient g0 [K, 4] (fp32; max|g0| = 1.5 exactly, in column 0), once per width, never modified."""
    c = indexed_case(dev, width, N=N_RAYS, S=N_SAMPLES)
    g0 = torch.randn(c.K, 4, generator=c.gen, dtype=torch.float64)
    i, j = divmod(int(g0.abs().argmax()), 4)
    big = float(g0[i, j])
    g0[i, j] = float(g0[i, 0])
    g0[i, 0] = big
    g0 = (g0 * (1.5 / abs(big))).float()
    g0[i, 0] = math.copysign(1.5, big)
    assert float(g0.abs().max()) == 1.5 and float(g0[:, 0].abs().max()) == 1.5
    c.g0, c.cap = g0, c.K + 17
    c.R = {m: E.pass_rows(m, width) for m in E.ALL_MODES}
    # 32-row tiles (chains) and row tiles of the f32 kernel each ray's listed rows fall into: two atomics commute, three need not
    rows = torch.arange(c.K)
    c.tiles_of_ray = {}
    for mode in E.ALL_MODES:
        unit = c.R["f32"] if mode == "f32" else 32
        n = torch.zeros(c.N, dtype=torch.long)
        for ray in range(c.N):
            n[ray] = (rows[c.idx[:, 0] == ray] // unit).unique().numel()
        c.tiles_of_ray[mode] = n
    return c


def d_out_of(c, k, dev):
    """g0 * 2^k on the listed entries of the [N, S, 4] grid, zero elsewhere (exact unless 2^k takes it below the fp32 normals)."""
    d_out = torch.zeros(c.N, c.S, 4, device=dev)
    d_out[c.idx[:, 0].to(dev), c.idx[:, 1].to(dev)] = (c.g0.double() * 2.0 ** k).float().to(dev)
    return d_out


def listed_rows(c, d_out):
    return d_out[c.idx[:, 0].to(d_out.device), c.idx[:, 1].to(d_out.device)]


def run(dev, c, mode, d_out, word, count=None):
    return run_chain(dev, c, mode, c.cap, c.K if count is None else count, d_out, word)


def outputs(c, r):
    """d_o, d_d and every parameter gradient of a run, fp64 on the CPU, by name."""
    ops = _ops()
    out = {"d_o": r.d_o.double().cpu(), "d_d": r.d_d.double().cpu()}
    for off, shp, name in zip(ops.param_offsets(c.net), c.net.shapes(), c.net.names()):
        out[name] = r.grads[off:off + int(np.prod(shp))].view(shp).double().cpu()
    return out


def autograd_reference(c, rows, masks=None):
    """fp64 autograd of the oracle over list entries [0, rows) with d_out = g0, on the fp32 sample positions the kernels form (z = zgrid +
    jitter, o + d z with separate fp32 roundings; the rounding enters as a constant, the derivative is that of o + d z)."""
    r_, j_ = c.idx[:rows, 0], c.idx[:rows, 1]
    p64 = {k: v.double().requires_grad_(True) for k, v in c.p.items()}
    d64, o64 = c.d.double().requires_grad_(True), c.o.double().requires_grad_(True)
    z = c.zg.unsqueeze(0) + c.jitter
    pos32 = c.o[r_] + c.d[r_] * z[r_, j_].unsqueeze(-1)
    pos = o64[r_] + d64[r_] * z.double()[r_, j_].unsqueeze(-1)
    pos = pos + (pos32.double() - pos).detach()
    enc = O.embed(pos, c.step_r, c.cfg)
    out = O.mlp_forward(p64, c.nc, enc, d64[r_]) if masks is None else masked_forward(p64, c.nc, enc, d64[r_], masks)
    (out * c.g0[:rows].double()).sum().backward()
    ref = {"d_o": o64.grad, "d_d": d64.grad}
    ref.update({name: p64[name].grad for name in c.net.names()})
    return ref


_REFS = {}


def reference(c, mode, r, rows=None):
    """The k = 0 autograd reference of `mode`: the oracle's own ReLU decisions (f32, f16x3, f16x3h), the kernel's (f16 / bf16, from the
    forward of run `r`: they do not depend on d_out).  Cached per (width, mode, rows)."""
    rows = c.K if rows is None else rows
    key = (c.nc.width, mode if mode in CHAINS16 else "plain", rows)
    if key not in _REFS:
        masks = None
        if mode in CHAINS16:
            masks = [m.double() for m in _ops().decode_masks_16(r.save.mask, c.nc.depth + 2, c.nc.width, rows)]
        _REFS[key] = autograd_reference(c, rows, masks)
        for name, v in _REFS[key].items():
            assert float(v.abs().max()) > 0, f"{name}: the reference gradient is zero, the comparison says nothing"
    return _REFS[key]


def gates(mode, ref):
    """The absolute gate of every output at k = 0 (module docstring); it scales by 2^k with the reference."""
    tol_ray = TOL_GRAD[mode] if mode in CHAINS16 else 1e-3
    top = {n: float(v.abs().max()) for n, v in ref.items()}
    gnet = max(v for n, v in top.items() if n not in ("d_o", "d_d"))
    g = {"d_o": tol_ray * top["d_o"], "d_d": tol_ray * top["d_d"]}
    for n in ref:
        if n in g:
            continue
        if mode in CHAINS16:
            g[n] = TOL_GRAD[mode] * top[n]
        elif mode == "f16x3h":
            g[n] = max(1e-3 * top[n], 5e-7 * gnet)
        else:
            g[n] = 2e-5 * (max(top[n], top[n[:-4] + "weight"]) if n.endswith(".bias") else top[n])
            if mode == "f16x3":                                       # the planes' quantum is relative to the launch's maximum (module docstring)
                g[n] = max(g[n], 5e-7 * gnet)
    return g


def compare(got, ref, gate):
    """One output tensor against its fp64 reference under the fp32 exclusions of the module docstring."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    a = ref.abs()
    sub, ovf = (a > 0) & (a < FLT_MIN), a > FLT_MAX
    exc = sub | ovf
    err = (got - ref).abs()
    within = err <= gate                                              # (NaN compares false)
    same_sign = torch.sign(got) == torch.sign(ref)
    ok = within | (sub & (got.abs() < FLT_MIN) & ((got == 0) | same_sign)) | (ovf & torch.isinf(got) & same_sign)
    finite = torch.isfinite(got) | ovf
    kept = err[~exc]
    top10 = torch.topk(a, min(10, a.numel())).indices
    return SimpleNamespace(ok=bool(ok.all()), bad=int((~ok).sum()), finite=bool(finite.all()), share=float(exc.double().mean()),
                           top_excluded=bool(exc[top10].any()), worst=float(kept.max()) if kept.numel() else 0.0, top=float(a.max()))


def sg_readable(mode, d_out_rows, sg):
    """Whether the largest |d_out[row, 0]| * SG survives the plane's 16-bit format: always in bf16 and f32, above the f16 subnormals'
    rounding noise (2^-17: 7 bits left) in the f16 planes."""
    return mode in ("f32", "bf16") or float(d_out_rows[:, 0].abs().max()) * sg >= 2.0 ** -17


def check_run(c, mode, r, d_out, word_value, k, over, tag, gated=True):
    """Everything (a) and (c) assert of one run: d_out = g0 * 2^k, the word `word_value` = max|d_out| * over (`over` = 1 where the word
    is not a finite number: SG = 1 then).  -> (failures, record line, worst error as a fraction of the true max|ref|)."""
    fails = []
    rows_out = listed_rows(c, d_out)
    sg = E.grad_scale(word_value)
    # ---- the scale the run used
    e_want = 0 if mode == "f32" else round(math.log2(sg))
    if sg_readable(mode, rows_out, 1.0 if mode == "f32" else sg):
        try:
            e_got = E.recover_scale(mode, r.dsh, rows_out)
            if e_got != e_want:
                fails.append(f"SG recovered 2^{e_got}, restated 2^{e_want}")
            sg_txt = f"2^{e_got}"
        except AssertionError as e:
            fails.append(str(e).splitlines()[0])
            sg_txt = "?"
    else:
        col = E.sigma_column(mode, r.dsh, c.K)
        if not bool((col == 0).all()):
            fails.append("dsh column 27 below the f16 range is not zero")
        sg_txt = f"n/a (restated 2^{e_want}; plane below the f16 range, zero)"
    # ---- parity
    ref0 = reference(c, mode, r)
    gate0 = gates(mode, ref0)
    got = outputs(c, r)
    s_ref, s_gate = 2.0 ** k, 2.0 ** k * over
    worst = {"d_o": 0.0, "d_d": 0.0, "dW": (0.0, "")}
    true_worst = 0.0
    share = 0.0
    for name, ref_t in ref0.items():
        q = compare(got[name], ref_t * s_ref, gate0[name] * s_gate)
        share = max(share, q.share)
        if not q.finite:
            fails.append(f"{name}: not finite")
        if gated and not q.ok:
            fails.append(f"{name}: {q.bad} entries past the gate, worst {q.worst / q.top:.2e} of max|ref| (gate {gate0[name] * s_gate / q.top:.1e})")
        if abs(k) <= 100 and (q.share > 0.01 or q.top_excluded):
            fails.append(f"{name}: {q.share:.2%} of the entries excluded, one of the 10 largest among them: {q.top_excluded}")
        frac = q.worst / q.top
        true_worst = max(true_worst, frac)
        if name in ("d_o", "d_d"):
            worst[name] = frac
        elif frac > worst["dW"][0]:
            worst["dW"] = (frac, name)
    # ---- dW against the GEMM of the operands its kernel read, decoded with the restated scale.  (An overstated word: the gate grows with
    #      it like the others.  The planes then hold a few bits per entry and many zeros, the GEMM is a sum of terms that cancel, and
    #      fp32 accumulation errs relative to the summands: measured 2e-7 of max|ref| at m = 1, 6e-6 .. 3e-5 at m = 20.)
    opnd = E.dw_reference(c.net.depth, c.nc.skips[0], E.operands(mode, c.net, r.save, r.dy, r.dsh, c.K, sg))
    w_op, w_op_name = 0.0, ""
    for name, want in opnd.items():
        want = want.view(got[name].shape)
        top = float(want.abs().max())
        q = compare(got[name], want, (2e-5 * top + 1e-9 * s_ref) * over)
        if gated and not q.ok:
            fails.append(f"{name} vs its operands: worst {q.worst:.3e}, max|ref| {top:.3e}")
        if top > 0 and q.worst / top > w_op:
            w_op, w_op_name = q.worst / top, name
    line = (f"[grad-range {tag}] SG {sg_txt} | of max|ref|: d_o {worst['d_o']:.1e} d_d {worst['d_d']:.1e} dW {worst['dW'][0]:.1e} ({worst['dW'][1]}); "
            f"dW vs its operands {w_op:.1e} ({w_op_name}) | excluded {share:.2%}" + ("" if gated else " | NOT GATED"))
    return fails, line, true_worst


# ------------------------------------------------------------------------------------------------------------------- (a) the sweep
@pytest.mark.parametrize("width,mode", PARAMS, ids=IDS)
def test_scale_sweep(gpu_device, width, mode):
    """d_out = g0 * 2^k, the word max|d_out|, k from -140 to 120: finite outputs, the recovered SG equal to the restated one, d_o / d_d /
    every dW within the mode's gates of the scaled fp64 reference and of the GEMM of its own operands.  k = -140 / -126: finite, SG (where
    the plane can hold it) 2^100, parity printed."""
    dev = gpu_device
    c = case(width, dev)
    failed = []
    for k in SWEEP:
        d_out = d_out_of(c, k, dev)
        wv = float(d_out.abs().max())
        assert wv == 1.5 * 2.0 ** k or k < -126
        r = run(dev, c, mode, d_out, word_of(wv, dev))
        fails, line, _ = check_run(c, mode, r, d_out, wv, k, 1.0, f"sweep {mode} W={width} k={k}", gated=k not in UNGATED)
        print(line)
        failed += [f"k={k}: {f}" for f in fails]
    assert not failed, f"[{mode} W={width}] " + " | ".join(failed)


# --------------------------------------------------------------------------------------------------------- (b) scale-free planes
@pytest.mark.parametrize("width,mode", PARAMS, ids=IDS)
def test_stored_planes_are_scale_free(gpu_device, width, mode):
    """The planes hold dY * SG and SG absorbs 2^k: dy and dsh over the covered tiles equal the k = 0 run's bit for bit in the four chain
    modes; in f32, dy(k) = dy(0) * 2^k bit for bit.  (f16x3h's planes are f16x3's hi planes at every k, too.)"""
    dev = gpu_device
    c = case(width, dev)
    D = c.nc.depth
    cov = E.covered_units(mode, c.K, c.R[mode])
    base = run(dev, c, mode, d_out_of(c, 0, dev), word_of(1.5, dev))
    planes = lambda r: [E.unit_bytes(mode, b, s, c.cap)[:, :cov].contiguous() for b, s in ((r.dy, D + 2), (r.dsh, 1))]
    b_dy, b_dsh = planes(base)
    for k in PLANE_KS:
        r = run(dev, c, mode, d_out_of(c, k, dev), word_of(1.5 * 2.0 ** k, dev))
        dy, dsh = planes(r)
        if mode == "f32":
            s = 2.0 ** k                                             # (exact in fp32; the product rounds only below the normals)
            assert torch.equal(dy.view(torch.float32), b_dy.view(torch.float32) * s), f"f32 k={k}: dy is not dy(0) * 2^k"
            assert torch.equal(dsh.view(torch.float32), b_dsh.view(torch.float32) * s), f"f32 k={k}: dsh is not dsh(0) * 2^k"
        else:
            ne = int((dy != b_dy).sum()), int((dsh != b_dsh).sum())
            assert ne == (0, 0), f"{mode} k={k}: {ne[0]} dy bytes and {ne[1]} dsh bytes differ from the k = 0 run's"
        if mode == "f16x3h":
            assert_planes_match(c, r, run(dev, c, "f16x3", d_out_of(c, k, dev), word_of(1.5 * 2.0 ** k, dev)), c.K)
    print(f"[grad-range planes {mode} W={width}] dy / dsh over {cov} units equal the k = 0 run's at k = {PLANE_KS}")


# ------------------------------------------------------------------------------------------------ (c) the word is an upper bound
@pytest.mark.parametrize("width,mode", PARAMS, ids=IDS)
def test_word_overstates_the_maximum(gpu_device, width, mode):
    """The fine pass back-propagates a listed subset while the word is the maximum over all of d_sig_rgb: d_out at k = 0, the word 2^m
    times its maximum.  SG is the restatement's for the WORD; every error stays within the gates taken of max|ref| * 2^m (the 16-bit
    quantum is fixed at 1 / SG); what the error is of the true max|ref| is printed, not gated."""
    dev = gpu_device
    c = case(width, dev)
    d_out = d_out_of(c, 0, dev)
    failed = []
    for m in OVERSTATED:
        wv = 1.5 * 2.0 ** m
        r = run(dev, c, mode, d_out, word_of(wv, dev))
        fails, line, true_worst = check_run(c, mode, r, d_out, wv, 0, 2.0 ** m, f"overstated {mode} W={width} m={m}")
        print(line + f" | worst error of the TRUE max|ref| {true_worst:.1e} (not gated)")
        failed += [f"m={m}: {f}" for f in fails]
    assert not failed, f"[{mode} W={width}] " + " | ".join(failed)


POWERS = (-96, -95, 0, 4, 100)


@pytest.mark.parametrize("width,mode", PARAMS, ids=IDS)
def test_words_at_and_beside_a_power_of_two(gpu_device, width, mode):
    """The word exactly 2^j and its two fp32 neighbours, where `ceilf(log2f(gmax))` decides the exponent: d_out = g0 * 2^(j - 1), so the
    word overstates max|d_out| = 0.75 * 2^j by 4/3.  The recovered SG is the restatement's, exactly: 2^(4 - j) at and below 2^j (2^100 at
    j = -96: the clamp and the formula meet there); above 2^j it is 2^(3 - j) only at j = 0: log2f is an fp32 function and returns j for
    the neighbour above 2^j at every |j| >= 2 (E.grad_scale), so the scale has not halved yet and word * SG = 2^4 (1 + 2^-23).  Both
    kernels take the same value (dW against its operands decoded with the restated SG).  Parity within the gates taken of max|ref| * 4/3.
    (At j = 4 the true log2 lies 0.36 ulp above 4: an fp32 log2f good to one ulp could return either neighbour; the device returns
    4, as rounding to nearest does.)"""
    dev = gpu_device
    c = case(width, dev)
    failed = []
    for j in POWERS:
        d_out = d_out_of(c, j - 1, dev)
        p2 = np.float32(2.0 ** j)
        for label, wv in (("below", float(np.nextafter(p2, np.float32(0)))), ("at", float(p2)), ("above", float(np.nextafter(p2, np.float32(np.inf))))):
            assert wv >= float(d_out.abs().max())
            r = run(dev, c, mode, d_out, word_of(wv, dev))
            fails, line, _ = check_run(c, mode, r, d_out, wv, j - 1, wv / (0.75 * 2.0 ** j), f"power {mode} W={width} word {label} 2^{j}")
            print(line)
            failed += [f"{label} 2^{j}: {f}" for f in fails]
    assert not failed, f"[{mode} W={width}] " + " | ".join(failed)


# ----------------------------------------------------------------------------------------------------------- (d) degenerate words
@pytest.mark.parametrize("width,mode", PARAMS, ids=IDS)
def test_degenerate_words(gpu_device, width, mode):
    """d_out = 0 with the word 0 (`gmax > 0.f` fails: SG = 1): every stored dy / dsh value over the covered tiles, d_o, d_d and every
    gradient is exactly zero.  Word bits of +inf, NaN and 3e38f (`gmax < 3e38f` fails: SG = 1) with an ordinary d_out: SG recovers as 1,
    the outputs are finite and within the gates."""
    dev = gpu_device
    c = case(width, dev)
    D = c.nc.depth
    cov = E.covered_units(mode, c.K, c.R[mode])
    r = run(dev, c, mode, torch.zeros(c.N, c.S, 4, device=dev), word_of(0.0, dev))
    dt = torch.float32 if mode == "f32" else (torch.bfloat16 if mode == "bf16" else torch.float16)
    for name, buf, slots in (("dy", r.dy, D + 2), ("dsh", r.dsh, 1)):
        v = E.unit_bytes(mode, buf, slots, c.cap)[:, :cov].contiguous().view(dt)
        assert bool((v == 0).all()), f"{mode} {name}: {int((v != 0).sum())} stored values not zero at d_out = 0 (NaN counts)"
    assert bool((r.d_o == 0).all()) and bool((r.d_d == 0).all()) and bool((r.grads == 0).all())
    d_out = d_out_of(c, 0, dev)
    failed = []
    for label, wv in (("+inf", float("inf")), ("NaN", float("nan")), ("3e38", 3e38)):
        r = run(dev, c, mode, d_out, word_of(wv, dev))
        fails, line, _ = check_run(c, mode, r, d_out, wv, 0, 1.0, f"word {label} {mode} W={width}")
        print(line)
        failed += [f"word {label}: {f}" for f in fails]
    assert not failed, f"[{mode} W={width}] " + " | ".join(failed)


# ------------------------------------------------------------------------------------------- (e) non-finite upstream gradients
def assert_other_rays_equal(c, mode, got, clean, skip_ray, tag):
    """d_o / d_d of every ray but `skip_ray`: bit for bit where a ray's rows fall into at most two tiles (two atomic addends commute),
    1e-6 max|.| elsewhere (module docstring)."""
    few = c.tiles_of_ray[mode] <= 2
    keep = torch.ones(c.N, dtype=torch.bool)
    if skip_ray is not None:
        keep[skip_ray] = False
    for name in ("d_o", "d_d"):
        a, b = getattr(got, name).cpu(), getattr(clean, name).cpu()
        assert torch.equal(a[keep & few], b[keep & few]), f"{tag} {name}: a ray other than {skip_ray} changed"
        assert bool(torch.isfinite(a[keep]).all()), f"{tag} {name}: a ray other than {skip_ray} is not finite"
        assert float((a[keep] - b[keep]).abs().max()) <= 1e-6 * float(b.abs().max()), f"{tag} {name}: a ray other than {skip_ray} changed"


@pytest.mark.parametrize("width,mode", PARAMS, ids=IDS)
def test_non_finite_gradients_are_not_swallowed(gpu_device, width, mode):
    """One LISTED row's d_out NaN, then +inf (the word: the finite maximum of the other rows, what composite_bwd leaves: it keeps a
    maximum only while < 3e38): that ray's d_o and d_d and at least one parameter gradient are non-finite, so the optimiser's check
    refuses the step; no other ray's d_o / d_d changes.  One UNLISTED grid entry and one list entry past the count NaN: every output
    equals the clean run's bit for bit, the weight gradients (float atomics) at 2e-5 of a tensor's maximum."""
    dev = gpu_device
    c = case(width, dev)
    clean_out = d_out_of(c, 0, dev)
    word = word_of(1.5, dev)
    clean = run(dev, c, mode, clean_out, word)
    assert bool(torch.isfinite(clean.grads).all()) and bool(torch.isfinite(clean.d_o).all()) and bool(torch.isfinite(clean.d_d).all())
    e = c.K // 2
    while float(c.g0[e].abs().max()) == 1.5:                         # (not the row that carries the maximum: the word stays what it is)
        e += 1
    ray, smp = int(c.idx[e, 0]), int(c.idx[e, 1])
    for label, bad in (("NaN", float("nan")), ("+inf", float("inf"))):
        d_out = clean_out.clone()
        d_out[ray, smp] = bad
        r = run(dev, c, mode, d_out, word)
        tag = f"{mode} W={width} listed {label}"
        assert not bool(torch.isfinite(r.grads).all()), f"{tag}: every parameter gradient is finite, the step would be taken"
        assert not bool(torch.isfinite(r.d_o[ray]).all()) and not bool(torch.isfinite(r.d_d[ray]).all()), f"{tag}: the ray's own gradient is finite"
        assert_other_rays_equal(c, mode, r, clean, ray, tag)
    # ---- unlisted: a grid entry that is not in the list, and the list's last entry with the count one short of it
    listed = torch.zeros(c.N, c.S, dtype=torch.bool)
    listed[c.idx[:, 0], c.idx[:, 1]] = True
    free = torch.nonzero(~listed)[len(torch.nonzero(~listed)) // 2]
    count = c.K - 1
    clean = run(dev, c, mode, clean_out, word, count=count)
    d_out = clean_out.clone()
    d_out[int(free[0]), int(free[1])] = float("nan")
    d_out[int(c.idx[c.K - 1, 0]), int(c.idx[c.K - 1, 1])] = float("nan")
    r = run(dev, c, mode, d_out, word, count=count)
    tag = f"{mode} W={width} unlisted NaN"
    assert torch.equal(r.out, clean.out)
    assert_other_rays_equal(c, mode, r, clean, None, tag)
    cov = E.covered_units(mode, count, c.R[mode])
    for (name, a, slots), (_, b, _) in zip(E.workspaces(c.net, r), E.workspaces(c.net, clean)):
        assert torch.equal(E.unit_bytes(mode, a, slots, c.cap)[:, :cov], E.unit_bytes(mode, b, slots, c.cap)[:, :cov]), f"{tag}: {name} changed"
    ga, gb = outputs(c, r), outputs(c, clean)
    worst = 0.0
    for name in c.net.names():
        top = float(gb[name].abs().max())
        err = float((ga[name] - gb[name]).abs().max())
        assert math.isfinite(err) and err <= 2e-5 * top, f"{tag} {name}: {err:.3e} of max {top:.3e}"
        worst = max(worst, err / top if top > 0 else 0.0)
    print(f"[grad-range non-finite {mode} W={width}] listed NaN / inf reach ray {ray} and the parameter gradients only; unlisted NaN: dW within {worst:.1e} of the clean run")


# ------------------------------------------------------------------------------------------------------------- 3: the model's own word
MODEL_FIXTURE = "g7_train_s32x2_deg1"


@pytest.mark.parametrize("precision", E.ALL_MODES)
def test_model_gradients_scale_with_the_loss(gpu_device, precision):
    """(c * loss).backward() through NeRF_Model for c = 2^-40, 1, 2^40: composite_bwd writes the word, the chains and the weight-gradient
    kernels read it.  Gradients / c against the c = 1 run: f32 and the split-f16 modes at the gates of
    tests/test_model_gpu.py::test_f16x3h_runs_the_f16x3_chains (ray gradients 1e-6 max|.|, a parameter tensor 1e-3 of its maximum or 5e-7
    of the net's; f32: 2e-5 of the tensor's maximum, module docstring), f16 / bf16 at TOL_GRAD of the whole gradient's maximum.  The
    fused RAdam takes the step at every c."""
    from conftest import load_golden, t
    from mc_nerf_amd.model import MC_NeRF_Loss, RAdam
    from test_model_gpu import build_model
    g = load_golden(MODEL_FIXTURE)
    dev = gpu_device
    res = {}
    for e in (0, -40, 40):
        m, cfg, pc, pf = build_model(g, dev, precision=precision)
        opt = RAdam(m.parameters(), lr=1e-3)
        d = t(g["rays_d"]).to(dev).requires_grad_(True)
        o = t(g["rays_o"]).to(dev).requires_grad_(True)
        rgb_c, rgb_f = m.render_rays_train(d, o, 0, float(g["step_r"]), jitter=t(g["jitter"]).to(dev), eps_c=t(g["eps_c"]).to(dev),
                                           eps_sel=t(g["eps_sel"]).to(dev), eps_f=t(g["eps_f"]).to(dev))
        loss = MC_NeRF_Loss(dict(data_img_h=800, data_img_w=800)).get_rgb_loss([rgb_c, rgb_f, t(g["gt"]).to(dev)])
        opt.zero_grad(set_to_none=True)
        (loss * 2.0 ** e).backward()
        grads = {f"{tag}.{k_}": p.grad.double().cpu() * 2.0 ** -e
                 for tag, net in (("c", m.nerf_coarse), ("f", m.nerf_fine)) for k_, p in net.named_parameters()}
        assert all(bool(torch.isfinite(v).all()) for v in grads.values())
        res[e] = (d.grad.double().cpu() * 2.0 ** -e, o.grad.double().cpu() * 2.0 ** -e, grads)
        opt.step()
        assert opt.skipped_steps() == 0, f"{precision} c=2^{e}: the step was refused"
    base = res[0]
    gnet = max(float(v.abs().max()) for v in base[2].values())
    assert gnet > 0 and float(base[0].abs().max()) > 0 and float(base[1].abs().max()) > 0
    for e in (-40, 40):
        got = res[e]
        ray_tol = TOL_GRAD[precision] if precision in CHAINS16 else 1e-6
        e_ray = max(float((got[i] - base[i]).abs().max()) / float(base[i].abs().max()) for i in (0, 1))
        assert e_ray <= ray_tol, (precision, e, e_ray)
        worst, bits = 0.0, True
        for k_, gb in base[2].items():
            err, top = float((got[2][k_] - gb).abs().max()), float(gb.abs().max())
            bits = bits and err == 0.0
            if precision == "f32" and k_.endswith(".bias"):          # (a signed sum over the rows: relative to its layer's weight gradient as well)
                top = max(top, float(base[2][k_[:-4] + "weight"].abs().max()))
            gate = TOL_GRAD[precision] * gnet if precision in CHAINS16 else (2e-5 * top if precision == "f32" else max(1e-3 * top, 5e-7 * gnet))
            assert err <= gate, (precision, e, k_, err, top, gnet)
            worst = max(worst, err / max(top, 5e-4 * gnet))
        print(f"[grad-range model {precision} c=2^{e}] ray gradients {e_ray:.1e} of max; parameter gradients / c vs c = 1: worst {worst:.1e} of a tensor's max"
              f" (bit-equal: {bits}); step taken")
