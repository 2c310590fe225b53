"""The regulariser library's kernels (csrc/distortion.hip, include/mcnerf_reg.h) on the GPU.

  parity        distortion_fwd and composite_bwd_w against the fp64 restatement tests/distortion_ref.py, on both input families of
                mask_ref ("a": the table's saturated / empty rays; "b": semi-transparent rays, where the term is live), at S = 2, 3, 63,
                64, 65, 129 (chunk edges), 1024 (LDS above 64 KiB), 2048 at 5 rays (the bound), one ray, and 8192 + 261 rays (grid
                stride), each in both depth forms and with white_back on and off.  Three outputs: dist; the backward with the case's
                d_rgb + d_fg + d_dist ("full"); the backward with d_rgb = 0 and d_fg = None, the distortion term alone ("alone").
                Bar per case and output: e_kernel <= 2 e_fp32 + 16 * 2^-24 * max|ref|, e_fp32 the fp32 restatement's own error on
                that case (mask_ref.bound).  An output whose reference is identically zero (the S = 2 rows: one duplicated depth) is
                not compared under that rule: |out| <= 1e-12.  The measured errors go to profiles/distortion_parity.txt.
                Measured on MI355X: all 80 variants pass; the semi-transparent rays at S = 1024 / 2048 sit at dist 1.2e-8 .. 1.5e-8
                (bars 4.6e-7 .. 1.7e-6), the full backward at 6.0e-8 .. 7.8e-8 (bars 2.1e-6 .. 3.5e-6), the term alone at
                5e-11 .. 1.6e-9 (bars 1.1e-9 .. 2.0e-8), with the suffix sum of the d_dist path in fp64;
  gmax          the gmax word equals max|d_sig_rgb|;
  bit identity  on every case of composite_ref.CASES, composite_bwd_w(d_fg = None, d_dist = None) is ops.composite_bwd and, with the
                case's d_fg only, ops.composite_bwd_front -- d_sig_rgb and the gmax word: the three libraries' instantiations of the
                backward's body (csrc/mcnerf_composite.h) are one computation;
  refusals      S = 2049 is refused with the output untouched, the forward accepts it; N = 0 gives empty results;
  determinism   two runs are torch.equal.
"""
import os

import pytest
import torch

import composite_ref as R
import distortion_ref as D
import mask_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _ops():
    from mc_nerf_amd import ops
    return ops


def _variant(shape, family, rows, wb, dev):
    """(host inputs, device inputs) of a variant: made once, shared, never written to."""
    key = (shape, family, rows, wb)
    if key not in _CACHE:
        inp = D.variant(shape, family, rows, wb)
        _CACHE[key] = (inp, {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()})
    return _CACHE[key]


def _depth_args(d):
    return (None, d["z"]) if d["z"].dim() == 2 else (d["z"], None)


def _record_parity(key, line):
    """profiles/distortion_parity.txt: one line per variant, rewritten by every run of the parity test."""
    path = os.path.join(ROOT, "profiles", "distortion_parity.txt")
    head = ("# distortion_fwd / composite_bwd_w (csrc/distortion.hip) against the fp64 restatement tests/distortion_ref.py; max abs error of the\n"
            "# kernel (e_k) beside the fp32 restatement's own (e_32) and the bar 2 e_32 + 16 * 2^-24 max|ref| (an identically-zero reference: 1e-12);\n"
            "# full: d_rgb + d_fg + d_dist, alone: d_dist only; written by tests/test_distortion_ops_gpu.py::test_parity_against_fp64\n")
    try:
        lines = {}
        if os.path.isfile(path):
            lines = {l.split(":")[0]: l for l in open(path).read().splitlines() if l and not l.startswith("#")}
        lines[key] = f"{key}: {line}"
        with open(path, "w") as f:
            f.write(head + "\n".join(lines[k] for k in sorted(lines)) + "\n")
    except OSError:                     # (a read-only checkout: the figures are still printed)
        pass


def _run(ops, d, white_back):
    grid, zr = _depth_args(d)
    dist, mom = ops.distortion_fwd(d["sig_rgb"], grid, d["jitter"], d["eps"], D.NEAR, D.FAR, z_rows=zr)
    full, gmax = ops.composite_bwd_w(d["sig_rgb"], grid, d["jitter"], d["eps"], d["d_rgb"], d["d_fg"], d["d_dist"], mom, D.NEAR, D.FAR,
                                     white_back, True, z_rows=zr)
    alone = ops.composite_bwd_w(d["sig_rgb"], grid, d["jitter"], d["eps"], torch.zeros_like(d["d_rgb"]), None, d["d_dist"], mom,
                                D.NEAR, D.FAR, white_back, z_rows=zr)
    return dist, mom, full, gmax, alone


@pytest.mark.parametrize("white_back", [True, False])
@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("shape", M.SHAPES)
def test_parity_against_fp64(gpu_device, shape, family, rows, white_back):
    ops = _ops()
    inp, d = _variant(shape, family, rows, white_back, gpu_device)
    dist, mom, full, gmax, alone = _run(ops, d, white_back)
    torch.cuda.synchronize()
    assert float(gmax.view(torch.float32).item()) == float(full.abs().max())               # (a maximum does not round)
    assert dist.shape == (inp["sig_rgb"].shape[0],) and mom.shape == (dist.shape[0], 16) and mom.dtype == torch.uint8
    ref, r32 = D.reference(inp, prefix=shape == "stride"), D.restated32(inp)
    rec, bad = [], []
    for name, g, k in (("dist", dist, "dist"), ("full", full, "d_full"), ("alone", alone, "d_alone")):
        rf = ref[k]
        assert tuple(g.shape) == tuple(rf.shape)
        (e_k, at), (e_32, _) = R.worst(g, rf), R.worst(r32[k], rf)
        zero = float(rf.abs().max()) == 0.0
        if zero:
            assert D.is_identically_zero(shape, rows), (shape, rows, name)
        bar = D.ZERO_TOL if zero else M.bound(e_32, rf)
        rec.append(f"{name} e_k {e_k:.3e} e_32 {e_32:.3e} bar {bar:.3e} max|ref| {float(rf.abs().max()):.3e}")
        if not e_k <= bar:
            bad.append(f"{rec[-1]} at {at}")
    if D.is_identically_zero(shape, rows):
        assert float(ref["dist"].abs().max()) == 0.0 and float(ref["d_alone"].abs().max()) == 0.0
    key = f"{shape} {family} {'rows' if rows else 'grid'} wb{int(white_back)}"
    print(f"[distortion parity, {key}] " + "; ".join(rec))
    _record_parity(key, "; ".join(rec))
    assert not bad, (key, bad)
    # the moments are the ray's (sum w, sum w s) in fp64
    w, s, _ = D.weights64(inp)
    m = mom.cpu().view(torch.float64)
    assert float((m[:, 0] - w.sum(1)).abs().max()) <= 1e-9 and float((m[:, 1] - (w * s).sum(1)).abs().max()) <= 1e-9
    if family == "b" and inp["sig_rgb"].shape[0] == 53 and inp["sig_rgb"].shape[1] >= 3:
        assert D.live_share(dist.cpu()) >= D.LIVE_SHARE
        assert float(ref["d_alone"].abs().max()) > D.LIVE_GRAD                # the term is live on these rays


@pytest.mark.parametrize("name", list(R.CASES))
def test_without_d_dist_the_backward_is_the_other_kernels_bits(gpu_device, name):
    ops = _ops()
    inp = R.make(name)
    d = {k: (v.to(gpu_device) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    grid, zr = _depth_args(d)
    g = torch.Generator().manual_seed(R.CASES[name]["seed"] + 77)
    d_fg = torch.randn(d["d_rgb"].shape[0], generator=g).to(gpu_device)
    args = (d["sig_rgb"], grid, d["jitter"], d["eps"], d["d_rgb"])
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    core, core_g = ops.composite_bwd(*args, d["white_back"], True, z_rows=zr)
    mine, mine_g = ops.composite_bwd_w(*args, None, None, None, D.NEAR, D.FAR, d["white_back"], True, z_rows=zr)
    front, front_g = ops.composite_bwd_front(*args, d_fg, d["white_back"], True, z_rows=zr)
    mine_f, mine_fg = ops.composite_bwd_w(*args, d_fg, None, None, D.NEAR, D.FAR, d["white_back"], True, z_rows=zr)
    torch.cuda.synchronize()
    assert same(mine, core), (name, int((mine.view(torch.int32) != core.view(torch.int32)).sum()))
    assert torch.equal(mine_g, core_g) and int(core_g.item()) != 0
    assert same(mine_f, front), (name, int((mine_f.view(torch.int32) != front.view(torch.int32)).sum()))
    assert torch.equal(mine_fg, front_g) and int(front_g.item()) != 0


def test_refusals_leave_the_output_untouched(gpu_device):
    from mc_nerf_amd import _reg
    from mc_nerf_amd._lib import McnerfError
    ops = _ops()
    N, S = 2, 2049
    sig, eps = torch.zeros(N, S, 4, device=gpu_device), torch.zeros(N, S, device=gpu_device)
    z, d_rgb, d_dist = torch.linspace(1, 8, S, device=gpu_device), torch.ones(N, 3, device=gpu_device), torch.ones(N, device=gpu_device)
    dist, mom = ops.distortion_fwd(sig, z, None, eps, 1.0, 8.0)               # (the forward has no LDS bound)
    assert dist.shape == (N,) and bool(torch.isfinite(dist).all())
    out = torch.full((N, S, 4), 7.0, device=gpu_device)
    with pytest.raises(McnerfError, match="mcnerf_reg_composite_bwd_w.*invalid argument"):
        _reg.call("mcnerf_reg_composite_bwd_w", sig, z, 0, None, eps, d_rgb, None, d_dist, mom, 1.0, 0.125, N, S, 1, out, None, ops._stream())
    with pytest.raises(McnerfError, match="mcnerf_reg_composite_bwd_w.*invalid argument"):      # d_dist without moments, at a legal S
        _reg.call("mcnerf_reg_composite_bwd_w", sig, z[:8].contiguous(), 0, None, eps, d_rgb, None, d_dist, None, 1.0, 0.125, N, 8, 1, out, None, ops._stream())
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    e = torch.zeros(0, 8, 4, device=gpu_device)                              # N = 0: empty results
    z8, e1 = z[:8].contiguous(), e[..., 0].contiguous()
    d0, m0 = ops.distortion_fwd(e, z8, None, e1, 1.0, 8.0)
    assert d0.shape == (0,) and m0.shape == (0, 16)
    assert ops.composite_bwd_w(e, z8, None, e1, e[:, 0, :3].contiguous(), None, d0, m0, 1.0, 8.0).shape == (0, 8, 4)


@pytest.mark.parametrize("shape, rows", [("edge_S129", True), ("lds_S1024", False), ("stride", True)])
def test_two_runs_give_the_same_bits(gpu_device, shape, rows):
    ops = _ops()
    _, d = _variant(shape, "b", rows, True, gpu_device)
    a, b = _run(ops, d, True), _run(ops, d, True)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
