"""Count edges and stale workspaces of the MLP kernels in the four precision modes tests/test_mlpx3h_gpu.py does not cover: "f32" (mlp_fwd /
mlp_bwd / mlp_dw.hip), "f16x3" (mlp_x3_*.hip) and "f16" / "bf16" (mlp16_*.hip): forward -> backward -> weight gradient over the first
`count` entries of a (ray, sample) list, `count` a device-side word at and around a tile, a weight-gradient slab, a pass, the capacity and
past it, and far below the capacity the grids were sized for.

Every workspace holds 0xFF bytes (NaN) before each launch, `out` 7.0, the gradients zero, so that what a kernel must not write is seen
intact and what it must write cannot be a left-over.  References: the CPU oracle in fp64 on the fp32 sample positions (forward), fp64
autograd of the oracle (ray gradients; f16 / bf16: with the kernel's own ReLU decisions), the fp64 GEMM of the very operands the
weight-gradient kernel read (tests/mlp_edges_ref.py), and the same launch with count = capacity, bit for bit: a row's result depends on
that row alone.  No mode is a reference for another.

The tail contract, from the kernel sources:
  * f32: nothing at or past row `count` is written.  mlp_fwd.hip `if (SAVE && ok) ... save + (size_t)(row0 + m) * WIDTH` with
    `ok = row0 + m < total`, mlp_bwd.hip mask_store `if (ok) *reinterpret_cast<f32x4*>(dysave + ...) = v;`, and mlp_dw.hip clamps its
    reads to the chunk (`rc = grow < r1 ? grow : r1 - 1`) and drops them (`if (base + row >= r1) a_c = AV(0.f);`).
  * chains: every wave of every pass that runs stores its whole 32-row tile; a lane past the count computes on a copy of the last listed
    row (`gc = valid ? g : total - 1`, so X is finite there) and its dY is exactly zero in every plane (mlp16_bwd.hip, mlp_x3_bwd.hip:
    `if (!valid) go = f32x4{0.f, 0.f, 0.f, 0.f};          // rows past the count contribute exactly zero everywhere`).  The weight-gradient
    kernels stream whole tiles (`ntiles = (rows + 31) / 32`) and are right only because of that zero.  Tiles behind the last pass that
    runs keep the fill.

Run with -s for the measured figures (profiles/mlp_edges_parity.txt).
"""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

import mlp_edges_ref as E
from oracle import mcnerf_oracle as O
from test_mlp16_gpu import TOL_FWD, TOL_GRAD, masked_forward
from test_mlpx3h_gpu import indexed_case, listed_mask, run_chain

pytestmark = pytest.mark.gpu

N_RAYS, N_SAMPLES = 29, 40


def _ops():
    from mc_nerf_amd import ops
    return ops


def chain16(mode):
    return mode in ("f16", "bf16")


def positions32(c, r_, j_):
    """Sample positions as every kernel forms them: z = zgrid + jitter, o + d z with separate fp32 roundings (model/mc_nerf.py:602)."""
    z = c.zg.unsqueeze(0) + c.jitter
    return c.o[r_] + c.d[r_] * z[r_, j_].unsqueeze(-1)


def oracle_out(c, rows):
    """The oracle's output on list entries `rows`, fp64 arithmetic on the fp32 sample positions."""
    r_, j_ = c.idx[rows, 0], c.idx[rows, 1]
    p64 = {k: v.double() for k, v in c.p.items()}
    with torch.no_grad():
        return O.mlp_forward(p64, c.nc, O.embed(positions32(c, r_, j_).double(), c.step_r, c.cfg), c.d[r_].double())


@lru_cache(maxsize=None)
def edge_case(width, dev):
    """The list of the count tests (N = 29, S = 40, 60 % listed, torch.nonzero order; net with a skip layer, BARF on), the output
    gradient (magnitudes of a mean-reduced loss) and the oracle's output on every entry: computed once per width, never modified."""
    c = indexed_case(dev, width, N=N_RAYS, S=N_SAMPLES)
    c.gout = torch.randn(c.K, 4, generator=c.gen) * 1e-4
    c.ref_out = oracle_out(c, slice(0, c.K))
    return c


def output_gradient(c, dev):
    d_out = torch.zeros(c.N, c.S, 4, device=dev)
    d_out[c.idx[:, 0].to(dev), c.idx[:, 1].to(dev)] = c.gout.to(dev)
    return d_out, d_out.abs().max().reshape(1).view(torch.int32), E.grad_scale(float(d_out.abs().max()))


def ray_gradient_reference(c, rows, masks=None):
    """fp64 autograd of the oracle over list entries [0, rows) -> (d_o, d_d) [N, 3]; `masks`: the ReLU decisions to take instead of the
    oracle's own (tests/test_mlp16_gpu.py::masked_forward)."""
    r_, j_ = c.idx[:rows, 0], c.idx[:rows, 1]
    p64 = {k: v.double() for k, v in c.p.items()}
    d64, o64 = c.d.double().requires_grad_(True), c.o.double().requires_grad_(True)
    z = (c.zg.unsqueeze(0) + c.jitter).double()
    enc = O.embed(o64[r_] + d64[r_] * z[r_, j_].unsqueeze(-1), c.step_r, c.cfg)
    ref = O.mlp_forward(p64, c.nc, enc, d64[r_]) if masks is None else masked_forward(p64, c.nc, enc, d64[r_], masks)
    (ref * c.gout[:rows].double()).sum().backward()
    return o64.grad, d64.grad


def check_forward(mode, c, r, rows, ref, sel=None):
    """`out` against the oracle on list entries [0, rows) (or the entries `sel` of them), 7.0 everywhere else.  -> the error in the
    mode's metric: absolute (f32 / f16x3, gate 2e-5), relative to max(1, max|ref|) (f16 / bf16, gate TOL_FWD)."""
    dev = r.out.device
    listed = listed_mask(c, rows, dev)
    assert int(listed.sum()) == rows
    assert bool((r.out[~listed] == 7.0).all()), "out written outside the first `count` list entries"
    ix = c.idx[:rows] if sel is None else c.idx[sel]
    got = r.out[ix[:, 0].to(dev), ix[:, 1].to(dev)].cpu().double()
    err = float((got - ref).abs().max())
    assert math.isfinite(err), "out not finite on the listed entries"
    if chain16(mode):
        err /= max(1.0, float(ref.abs().max()))
        assert err < TOL_FWD[mode], (mode, err)
    else:
        assert err < 2e-5, (mode, err)
    return err


def check_tail(mode, c, r, rows, cap, R, bwd=True):
    """The tail contract of the module docstring, on the workspaces of run `r` over `rows` rows."""
    net, W = c.net, c.nc.width
    spaces = [s for s in E.workspaces(net, r) if bwd or s[0] not in ("dy", "dsh")]
    behind = E.covered_units(mode, rows, R)
    for name, buf, slots in spaces:
        tail = E.unit_bytes(mode, buf, slots, cap)[:, behind:]
        assert bool((tail == E.FILL).all()), f"{mode} {name}: written at or behind unit {behind} (rows {rows}, {R} per pass)"
    if mode == "f32" or rows % 32 == 0:
        return
    t_, r0 = rows // 32, rows % 32
    for name, buf, slots, width in (("act", r.save.act, net.depth + 2, W), ("enc", r.save.enc, 1, 64)):
        x = E.tile_planes(mode, buf, slots, width, t_)[..., r0:, :]
        assert bool(torch.isfinite(x).all()), f"{mode} {name} rows {rows} .. {32 * t_ + 31}: not finite"
    if not bwd:
        return
    for name, buf, slots, width in (("dy", r.dy, net.depth + 2, W), ("dsh", r.dsh, 1, 32)):
        g = E.tile_planes(mode, buf, slots, width, t_)[..., r0:, :]
        assert bool((g == 0).all()), f"{mode} {name} rows {rows} .. {32 * t_ + 31}: {int((g != 0).sum())} stored values not zero (NaN counts)"


def check_dw(mode, c, r, rows, sg, tag):
    """Every weight gradient against the fp64 GEMM of rows [0, rows) of its own operands: 2e-5 max|ref| + 1e-9 per tensor, the gate of
    test_mlp_dw_at_scale / test_x3_dw_at_scale / test_mlp16_dw_at_scale (f16 and bf16 products are exact in fp32, the split-f16 ones
    good to 2^-21: summation order is all that is left).  -> the worst error as a fraction of max|ref|."""
    ops = _ops()
    net = c.net
    ref = E.dw_reference(net.depth, c.nc.skips[0], E.operands(mode, net, r.save, r.dy, r.dsh, rows, sg))
    worst, worst_name = 0.0, ""
    for off, shp, name in zip(ops.param_offsets(net), net.shapes(), net.names()):
        n = int(np.prod(shp))
        got = r.grads[off:off + n].view(shp).double().cpu()
        want = ref[name].view(shp)
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        assert math.isfinite(err) and err <= 2e-5 * scale + 1e-9, f"{tag} {name}: err {err:.3e}, max|ref| {scale:.3e}"
        if scale > 0 and err / scale > worst:
            worst, worst_name = err / scale, name
    return worst, worst_name


def check_ray_gradients(mode, c, r, rows):
    """d_o / d_d against fp64 autograd over list entries [0, rows).  f32 / f16x3: 2e-5 max(1, max|ref|).  f16 / bf16: the reference takes
    the kernel's ReLU decisions, TOL_GRAD relative to max|ref|.  max|ref| is asserted not to be zero.  -> the two errors as fractions of
    max|ref|."""
    ops = _ops()
    if chain16(mode):
        masks = [m.double() for m in ops.decode_masks_16(r.save.mask, c.nc.depth + 2, c.nc.width, rows)]
        ref_o, ref_d = ray_gradient_reference(c, rows, masks)
    else:
        ref_o, ref_d = ray_gradient_reference(c, rows)
    errs = []
    for name, got, ref in (("d_o", r.d_o, ref_o), ("d_d", r.d_d, ref_d)):
        scale = float(ref.abs().max())
        assert scale > 0, f"{name}: the reference gradient over {rows} rows is zero, the comparison says nothing"
        err = float((got.cpu().double() - ref).abs().max())
        assert math.isfinite(err)
        if chain16(mode):
            assert err / scale < TOL_GRAD[mode], (mode, name, err, scale)
        else:
            assert err < 2e-5 * max(1.0, scale), (mode, name, err, scale)
            # That gate is absolute at these gradient magnitudes (max|ref| about 1e-5): it would let a missing gradient pass.  So, beside
            # it, 1e-3 of max|ref|.  The reference's positions are fp64, the kernel's fp32: half an ulp of |x| <= 4, 2.4e-7, times 2^5
            # (BARF at this step passes frequencies 0 .. 5) is a phase error below 1e-5, and fp32 accumulation adds about 1e-6: 1e-3
            # leaves a factor of 50 and is still a twentieth of what one dropped sample of a 20-sample ray moves.
            assert err < 1e-3 * scale, (mode, name, err, scale)
        errs.append(err / scale)
    return errs


def check_all(mode, c, r, rows, cap, R, sg, tag):
    """Forward, tail contract, dW, ray gradients of one run over `rows` (already clamped) rows.  Each of the four is run whatever the
    others say, so that a failure names everything that broke; the measured figures are printed when all hold."""
    checks = (("forward", lambda: check_forward(mode, c, r, rows, c.ref_out[:rows])), ("tail contract", lambda: check_tail(mode, c, r, rows, cap, R)),
              ("dW", lambda: check_dw(mode, c, r, rows, sg, tag)), ("ray gradients", lambda: check_ray_gradients(mode, c, r, rows)))
    got, failed = {}, []
    for name, check in checks:
        try:
            got[name] = check()
        except AssertionError as e:
            failed.append(f"{name}: {str(e).splitlines()[0]}")              # (the message itself, without pytest's expansion of the values)
    assert not failed, f"[edges {tag}] " + " | ".join(failed)
    e_out, (worst, worst_name), (e_o, e_d) = got["forward"], got["dW"], got["ray gradients"]
    print(f"[edges {tag}] out {e_out:.1e}; dW vs fp64 GEMM of its operands: worst {worst:.1e} of max|ref| ({worst_name}); d_o {e_o:.1e} d_d {e_d:.1e} of max|ref|")


def edge_counts(mode):
    return ["1"] + (["15", "16", "17"] if mode == "f32" else []) + ["31", "32", "33", "R-1", "R", "R+1", "cap", "cap+1000"]


EDGE_PARAMS = [(m, e) for m in E.MODES for e in edge_counts(m)]


@pytest.mark.parametrize("width", [64, 256])
@pytest.mark.parametrize("mode,edge", EDGE_PARAMS, ids=[f"{m}-{e}" for m, e in EDGE_PARAMS])
def test_count_edges(gpu_device, width, mode, edge):
    """Device-side counts around a tile (32), a weight-gradient slab of the f32 kernel (16), a pass (R), at the capacity 2 R + 64 and 1000
    past it (the `min(*count, max_rows)` clamp: exactly the launch with count = capacity).  Forward against the oracle and untouched
    elsewhere; the same rows bit for bit when the launch runs over the whole capacity; the tail contract; dW against the GEMM of its own
    operands; ray gradients against fp64 autograd."""
    dev = gpu_device
    R = E.pass_rows(mode, width)
    cap = 2 * R + 64
    count = {"R-1": R - 1, "R": R, "R+1": R + 1, "cap": cap, "cap+1000": cap + 1000}.get(edge) or int(edge)
    rows = min(count, cap)
    c = edge_case(width, dev)
    assert c.K >= cap, (c.K, cap)
    d_out, gmax, sg = output_gradient(c, dev)
    r = run_chain(dev, c, mode, cap, count, d_out, gmax)
    check_all(mode, c, r, rows, cap, R, sg, f"count {mode} W={width} count={edge}")
    # ---- count invariance: the forward over the whole capacity gives these rows, and the units wholly below `rows`, the same bits
    full = run_chain(dev, c, mode, cap, cap, d_out, gmax, bwd=False)
    ix = c.idx[:rows].to(dev)
    assert torch.equal(r.out[ix[:, 0], ix[:, 1]], full.out[ix[:, 0], ix[:, 1]]), "out of the first `count` entries depends on the count"
    whole = rows // E.unit_rows(mode)
    for (name, a, slots), (_, b, _) in zip(E.workspaces(c.net, r)[:4], E.workspaces(c.net, full)[:4]):
        ua, ub = E.unit_bytes(mode, a, slots, cap), E.unit_bytes(mode, b, slots, cap)
        assert torch.equal(ua[:, :whole], ub[:, :whole]), f"{mode} {name}: units below row {rows} depend on the count"
        if count > cap:
            assert torch.equal(ua, ub), f"{mode} {name}: count = capacity + 1000 is not the launch with count = capacity"
    if count > cap:
        assert torch.equal(r.out, full.out)


@pytest.mark.parametrize("width", [64, 256])
@pytest.mark.parametrize("mode", E.MODES)
def test_count_zero(gpu_device, width, mode):
    """count = 0: every kernel returns at its entry guard, before any row index is clamped to count - 1.  Nothing is written anywhere."""
    dev = gpu_device
    cap = 2 * E.pass_rows(mode, width) + 64
    c = edge_case(width, dev)
    d_out, gmax, _ = output_gradient(c, dev)
    r = run_chain(dev, c, mode, cap, 0, d_out, gmax)
    assert bool((r.out == 7.0).all())
    assert bool((r.grads == 0).all()) and bool((r.d_o == 0).all()) and bool((r.d_d == 0).all())
    for name, buf, _ in E.workspaces(c.net, r):
        assert bool((buf.view(torch.uint8) == E.FILL).all()), f"{mode} {name}: written at count = 0"


@pytest.mark.parametrize("width", [64, 256])
@pytest.mark.parametrize("edge", ["33", "R+1"])
@pytest.mark.parametrize("mode", E.MODES)
def test_small_count_under_large_capacity(gpu_device, width, mode, edge):
    """The fine pass early in training: capacity C R + 64 on C compute units, so every persistent grid is full, and a count of one or two
    tiles: all workgroups but the first find an empty range (`row0 >= total`, `r0 >= rows` in dw_kernel, `t0 >= t1` in the stream
    kernels) and must leave everything alone."""
    dev = gpu_device
    C = torch.cuda.get_device_properties(dev).multi_processor_count
    R = E.pass_rows(mode, width)
    cap = C * R + 64
    count = R + 1 if edge == "R+1" else int(edge)
    c = edge_case(width, dev)
    assert c.K >= count
    d_out, gmax, sg = output_gradient(c, dev)
    r = run_chain(dev, c, mode, cap, count, d_out, gmax)
    check_all(mode, c, r, count, cap, R, sg, f"large-cap {mode} W={width} cap={cap} count={edge}")


@pytest.mark.parametrize("width", [32, 64, 128, 256])
@pytest.mark.parametrize("mode", E.MODES)
def test_multi_pass_ragged(gpu_device, width, mode):
    """3 C R + 37 listed rows on C compute units (R rows per pass): every workgroup of the forward / backward runs three passes and the
    first a fourth, ragged one; the weight-gradient kernels stream tens of tiles or slabs per workgroup.  Oracle on 4000 random rows,
    dW against the GEMM of its own operands (on the device), the tail contract."""
    dev = gpu_device
    C = torch.cuda.get_device_properties(dev).multi_processor_count
    R = E.pass_rows(mode, width)
    K = 3 * C * R + 37
    S = 64
    N = -(-K // int(S * 0.55))                                 # 60 % of the grid is listed: enough for K entries
    c = indexed_case(dev, width, N=N, S=S, K=K, seed=1)
    cap = K + 64
    d_out = torch.randn(N, S, 4, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 1e-4
    gmax, sg = d_out.abs().max().reshape(1).view(torch.int32), E.grad_scale(float(d_out.abs().max()))
    r = run_chain(dev, c, mode, cap, K, d_out, gmax)
    sub = torch.randperm(K, generator=c.gen)[:4000]
    e_out = check_forward(mode, c, r, K, oracle_out(c, sub), sel=sub)
    check_tail(mode, c, r, K, cap, R)
    worst, worst_name = check_dw(mode, c, r, K, sg, f"{mode} W={width}")
    print(f"[edges multi-pass {mode} W={width}] {C} CUs, {K} rows: out {e_out:.1e}; dW vs fp64 GEMM of its operands: worst {worst:.1e} of max|ref| "
          f"({worst_name})")
