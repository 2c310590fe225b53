"""The geometry library's kernels (csrc/depth.hip, include/mcnerf_geo.h) on the GPU.

  parity        expected_depth and composite_bwd_z against the fp64 restatement tests/depth_ref.py, on both input families of mask_ref
                ("a": the table's saturated / empty rays; "b": semi-transparent rays), at S = 2, 3, 63, 64, 65, 129 (chunk edges),
                1024 (LDS above 64 KiB), 2048 at 5 rays (the bound), one ray, and 8192 + 261 rays (grid stride), each in both depth
                forms and with white_back on and off.  Outputs: zexp; the backward with d_rgb + d_zexp ("rz"); the backward with
                d_rgb = 0 and d_zexp alone ("z"); on the S = 65 / 129 / 1024 shapes the backward with all four gradients ("all").
                Bar per case and output: e_kernel <= 2 e_fp32 + 16 * 2^-24 * max|ref|, e_fp32 the fp32 restatement's own error on
                that case (mask_ref.bound).  The measured errors go to profiles/depth_parity.txt.
                Measured on MI355X: all 80 variants pass, no output above 0.16 of its bar; the semi-transparent rays at S = 1024 / 2048
                sit at zexp 1.2e-7 .. 2.4e-7 (bars 1.2e-5 .. 1.5e-5), rz 6.0e-8 .. 7.8e-8 (bars 2.1e-6 .. 3.5e-6), z 7e-10 .. 1.2e-8
                (bars 8.0e-9 .. 1.5e-6);
  gmax          the gmax word equals max|d_sig_rgb|;
  bit identity  on every case of composite_ref.CASES, composite_bwd_z(d_zexp = None) is ops.composite_bwd_w -- d_sig_rgb and the gmax
                word -- with neither, either and both of d_fg / d_dist: the four libraries' instantiations of the backward's body
                (csrc/mcnerf_composite.h) are one computation;
  refusals      leave a 7.0-prefilled output untouched; the forward has no bound on S; N = 0 gives empty results;
  determinism   two runs of all four ops are torch.equal;
  gather_depth  against indexing, C = 3, H W = 37 * 53, K = 1 and K = 3 (cameras [2, 0, 2]), n = 1000 / 1 / 5; stored 0, -1, NaN,
                +-inf and pixel ids -1 and HW give 0;
  depth_loss    n = 1, 5, 1000, 8453 with no, exactly one and every ray valid, with and without zexp_f: value <= 2e-6 max(1, |ref|),
                gradients <= 2e-6 max|ref| against fp64 (the bars tests/test_mask_ops_gpu.py holds mask_loss to); invalid rays'
                gradients are exactly zero; the all-invalid case is exactly zero without NaN; the counter word is zero on exit.
"""
import os

import pytest
import torch

import composite_ref as R
import depth_ref as Z
import distortion_ref as D
import mask_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD, LOSS = "mcnerf_geo_depth_fwd", "mcnerf_geo_composite_bwd_z", "mcnerf_geo_depth_loss"
_CACHE = {}


def _ops():
    from mc_nerf_amd import ops
    return ops


def _variant(shape, family, rows, wb, dev):
    """(host inputs, device inputs) of a variant: made once, shared, never written to."""
    key = (shape, family, rows, wb)
    if key not in _CACHE:
        inp = Z.variant(shape, family, rows, wb)
        _CACHE[key] = (inp, {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()})
    return _CACHE[key]


def _depth_args(d):
    return (None, d["z"]) if d["z"].dim() == 2 else (d["z"], None)


def _record_parity(key, line):
    """profiles/depth_parity.txt: one line per variant, rewritten by every run of the parity test."""
    path = os.path.join(ROOT, "profiles", "depth_parity.txt")
    head = ("# expected_depth / composite_bwd_z (csrc/depth.hip) against the fp64 restatement tests/depth_ref.py; max abs error of the kernel\n"
            "# (e_k) beside the fp32 restatement's own (e_32) and the bar 2 e_32 + 16 * 2^-24 max|ref|; rz: d_rgb + d_zexp, z: d_zexp only,\n"
            "# all: d_rgb + d_fg + d_dist + d_zexp; written by tests/test_depth_ops_gpu.py::test_parity_against_fp64\n")
    try:
        lines = {}
        if os.path.isfile(path):
            lines = {l.split(":")[0]: l for l in open(path).read().splitlines() if l and not l.startswith("#")}
        lines[key] = f"{key}: {line}"
        with open(path, "w") as f:
            f.write(head + "\n".join(lines[k] for k in sorted(lines)) + "\n")
    except OSError:                     # (a read-only checkout: the figures are still printed)
        pass


def _run(ops, d, white_back, all_four):
    grid, zr = _depth_args(d)
    args = (d["sig_rgb"], grid, d["jitter"], d["eps"])
    zexp = ops.expected_depth(*args, z_rows=zr)
    rz, gmax = ops.composite_bwd_z(*args, d["d_rgb"], None, None, None, d["d_zexp"], D.NEAR, D.FAR, white_back, True, z_rows=zr)
    z = ops.composite_bwd_z(*args, torch.zeros_like(d["d_rgb"]), None, None, None, d["d_zexp"], D.NEAR, D.FAR, white_back, z_rows=zr)
    out = [zexp, rz, gmax, z]
    if all_four:
        _, mom = ops.distortion_fwd(*args, D.NEAR, D.FAR, z_rows=zr)
        out += list(ops.composite_bwd_z(*args, d["d_rgb"], d["d_fg"], d["d_dist"], mom, d["d_zexp"], D.NEAR, D.FAR, white_back, True, z_rows=zr))
    return out


@pytest.mark.parametrize("white_back", [True, False])
@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("shape", M.SHAPES)
def test_parity_against_fp64(gpu_device, shape, family, rows, white_back):
    ops = _ops()
    all_four = shape in Z.ALL_FOUR
    inp, d = _variant(shape, family, rows, white_back, gpu_device)
    zexp, rz, gmax, z, *rest = _run(ops, d, white_back, all_four)
    torch.cuda.synchronize()
    assert float(gmax.view(torch.float32).item()) == float(rz.abs().max())                 # (a maximum does not round)
    assert zexp.shape == (inp["sig_rgb"].shape[0],) and zexp.dtype == torch.float32
    ref, r32 = Z.reference(inp, all_four), Z.restated32(inp, all_four)
    outputs = [("zexp", zexp, "zexp"), ("rz", rz, "d_rz"), ("z", z, "d_z")]
    if all_four:
        assert float(rest[1].view(torch.float32).item()) == float(rest[0].abs().max())
        outputs.append(("all", rest[0], "d_all"))
    rec, bad = [], []
    for name, g, k in outputs:
        rf = ref[k]
        assert tuple(g.shape) == tuple(rf.shape)
        (e_k, at), (e_32, _) = R.worst(g, rf), R.worst(r32[k], rf)
        bar = M.bound(e_32, rf)
        rec.append(f"{name} e_k {e_k:.3e} e_32 {e_32:.3e} bar {bar:.3e} max|ref| {float(rf.abs().max()):.3e}")
        if not e_k <= bar:
            bad.append(f"{rec[-1]} at {at}")
    key = f"{shape} {family} {'rows' if rows else 'grid'} wb{int(white_back)}"
    print(f"[depth parity, {key}] " + "; ".join(rec))
    _record_parity(key, "; ".join(rec))
    assert not bad, (key, bad)
    assert float(ref["d_z"].abs().max()) > 0.0                                 # the term is live on every variant
    if family == "b" and inp["sig_rgb"].shape[0] == 53 and inp["sig_rgb"].shape[1] >= 3:
        assert float(ref["d_z"].abs().max()) > 1e-3


@pytest.mark.parametrize("name", list(R.CASES))
def test_without_d_zexp_the_backward_is_the_regulariser_kernels_bits(gpu_device, name):
    ops = _ops()
    inp = R.make(name)
    d = {k: (v.to(gpu_device) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    grid, zr = _depth_args(d)
    g = torch.Generator().manual_seed(R.CASES[name]["seed"] + 77)
    N = d["d_rgb"].shape[0]
    d_fg, d_dist = torch.randn(N, generator=g).to(gpu_device), torch.randn(N, generator=g).to(gpu_device)
    args = (d["sig_rgb"], grid, d["jitter"], d["eps"])
    _, mom = ops.distortion_fwd(*args, D.NEAR, D.FAR, z_rows=zr)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    for fg, dist in ((None, None), (d_fg, None), (None, d_dist), (d_fg, d_dist)):
        m = mom if dist is not None else None
        want, want_g = ops.composite_bwd_w(*args, d["d_rgb"], fg, dist, m, D.NEAR, D.FAR, d["white_back"], True, z_rows=zr)
        mine, mine_g = ops.composite_bwd_z(*args, d["d_rgb"], fg, dist, m, None, D.NEAR, D.FAR, d["white_back"], True, z_rows=zr)
        torch.cuda.synchronize()
        assert same(mine, want), (name, fg is not None, dist is not None, int((mine.view(torch.int32) != want.view(torch.int32)).sum()))
        assert torch.equal(mine_g, want_g) and int(want_g.item()) != 0
    core, core_g = ops.composite_bwd(*args, d["d_rgb"], d["white_back"], True, z_rows=zr)       # with everything None: the core's bits
    mine, mine_g = ops.composite_bwd_z(*args, d["d_rgb"], None, None, None, None, D.NEAR, D.FAR, d["white_back"], True, z_rows=zr)
    assert same(mine, core) and torch.equal(mine_g, core_g)


def test_refusals_leave_the_output_untouched(gpu_device):
    from mc_nerf_amd import _geo
    from mc_nerf_amd._lib import McnerfError
    ops = _ops()
    N, S = 2, 2049
    sig, eps = torch.zeros(N, S, 4, device=gpu_device), torch.zeros(N, S, device=gpu_device)
    z, d_rgb, d_z = torch.linspace(1, 8, S, device=gpu_device), torch.ones(N, 3, device=gpu_device), torch.ones(N, device=gpu_device)
    zexp = ops.expected_depth(sig, z, None, eps)                              # (the forward has no bound on S)
    assert zexp.shape == (N,) and bool(torch.isfinite(zexp).all()) and float(zexp.min()) >= 1.0 and float(zexp.max()) <= 8.0
    out = torch.full((N, S, 4), 7.0, device=gpu_device)
    st = ops._stream()
    z8 = z[:8].contiguous()
    mom = torch.zeros(N, 16, dtype=torch.uint8, device=gpu_device)
    refused = [
        (BWD, (sig, z, 0, None, eps, d_rgb, None, None, None, d_z, 1.0, 0.125, N, S, 1, out, None, st)),          # S over the bound
        (BWD, (sig, z8, 5, None, eps, d_rgb, None, None, None, d_z, 1.0, 0.125, N, 8, 1, out, None, st)),         # z_stride neither 0 nor S
        (BWD, (sig, z8, 0, None, eps, d_rgb, None, d_z, None, d_z, 1.0, 0.125, N, 8, 1, out, None, st)),          # d_dist without moments
        (BWD, (sig, z8, 0, None, eps, d_rgb, None, None, mom, d_z, 1.0, 0.125, N, 8, 1, out, None, st)),          # moments without d_dist
        (BWD, (sig, z8, 0, None, eps, d_rgb, None, d_z, mom, d_z, 1.0, float("inf"), N, 8, 1, out, None, st)),    # non-finite span with d_dist
        (BWD, (sig, z8, 0, None, eps, None, None, None, None, d_z, 1.0, 0.125, N, 8, 1, out, None, st)),          # null d_rgb
        (BWD, (sig, z8, 0, None, eps, d_rgb, None, None, None, d_z, 1.0, 0.125, 1 << 21, 1 << 10, 1, out, None, st)),   # N S >= 2^31
        (FWD, (sig, z8, 3, None, eps, N, 8, out, st)),                                                             # z_stride neither 0 nor S
        (FWD, (sig, None, 0, None, eps, N, 8, out, st)),                                                           # null zgrid
        (LOSS, (d_z, None, d_z, N, 1.0, 0.125, -1.0, out, out, None, st)),                                         # negative weight
        (LOSS, (d_z, None, d_z, N, 1.0, float("nan"), 0.5, out, out, None, st)),                                   # non-finite z_scale
        (LOSS, (d_z, None, d_z, -1, 1.0, 0.125, 0.5, out, out, None, st)),                                         # n < 0
        (LOSS, (d_z, d_z, d_z, N, 1.0, 0.125, 0.5, out, out, None, st)),                                           # zexp_f without d_f
    ]
    for name, args in refused:
        with pytest.raises(McnerfError, match=name + ".*invalid argument"):
            _geo.call(name, *args)
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    pix = torch.zeros(4, dtype=torch.int64, device=gpu_device)
    depth = torch.ones(3, 10, device=gpu_device)
    for cams, seg in (([3], [0, 4]), ([-1], [0, 4]), ([0, 1], [0, 6, 4]), ([0], [1, 4]), ([0] * 65, list(range(65)) + [4])):
        with pytest.raises(McnerfError):
            ops.gather_depth(depth, cams, seg, pix)
    e = torch.zeros(0, 8, 4, device=gpu_device)                              # N = 0: empty results
    e1 = e[..., 0].contiguous()
    assert ops.expected_depth(e, z8, None, e1).shape == (0,)
    assert ops.composite_bwd_z(e, z8, None, e1, e[:, 0, :3].contiguous(), None, None, None, e[:, 0, 0].contiguous(), 1.0, 8.0).shape == (0, 8, 4)
    assert ops.gather_depth(depth, [0], [0, 0], pix[:0]).shape == (0,)


@pytest.mark.parametrize("shape, rows", [("edge_S129", True), ("lds_S1024", False), ("stride", True)])
def test_two_runs_give_the_same_bits(gpu_device, shape, rows):
    ops = _ops()
    _, d = _variant(shape, "b", rows, True, gpu_device)
    a, b = _run(ops, d, True, True), _run(ops, d, True, True)
    torch.cuda.synchronize()
    assert len(a) == 6
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    g = torch.Generator().manual_seed(9)
    depth, pix = _depth_images(gpu_device), torch.randint(0, HW, (1000,), generator=g).to(gpu_device)
    assert torch.equal(ops.gather_depth(depth, [2, 0, 2], [0, 300, 300, 1000], pix), ops.gather_depth(depth, [2, 0, 2], [0, 300, 300, 1000], pix))


# ------------------------------------------------------------------------------------------------------------------ gather_depth
HW = 37 * 53
SPECIAL = (0.0, -1.0, float("nan"), float("inf"), -float("inf"))


def _depth_images(dev):
    """[3, 37 * 53] targets in (0.5, 8); pixels 0 .. 4 of every camera hold 0, -1, NaN, +inf, -inf; the last pixel is valid."""
    g = torch.Generator().manual_seed(21)
    depth = 0.5 + 7.5 * torch.rand(3, HW, generator=g)
    depth[:, :5] = torch.tensor(SPECIAL)
    return depth.to(dev)


@pytest.mark.parametrize("cams, seg", [([1], [0, 1000]), ([2, 0, 2], [0, 300, 300, 1000]), ([2, 0, 2], [0, 333, 667, 1000]), ([1], [0, 1]), ([2], [0, 5]),
                                       ([2, 0, 2], [0, 2, 3, 5]), ([2, 0, 2], [0, 0, 1, 1])])
def test_gather_depth_is_the_indexed_value_or_zero(gpu_device, cams, seg):
    ops = _ops()
    depth = _depth_images(gpu_device)
    n = seg[-1]
    g = torch.Generator().manual_seed(22 + n)
    pix = torch.randint(0, HW, (n,), generator=g)
    if n >= 5:
        pix[:5] = torch.arange(5)                                            # the stored 0, -1, NaN, +inf, -inf
    if n >= 1000:
        pix[-6:-1], pix[-1] = torch.arange(5), HW - 1                        # ... in the last segment too, and the last pixel
        pix[500], pix[501], pix[502], pix[503] = -1, HW, -(1 << 40), 1 << 40      # ids outside the image
    pix = pix.to(gpu_device)
    got = ops.gather_depth(depth, cams, seg, pix)
    cam_of = torch.cat([torch.full((hi - lo,), c, dtype=torch.int64) for c, lo, hi in zip(cams, seg, seg[1:])]).to(gpu_device)
    inside = (pix >= 0) & (pix < HW)
    v = depth[cam_of, pix.clamp(0, HW - 1)]
    want = torch.where(inside & torch.isfinite(v) & (v > 0), v, torch.zeros_like(v))
    assert got.dtype == torch.float32 and got.shape == (n,) and torch.equal(got, want)
    assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0
    if n >= 5:
        assert got[:5].tolist() == [0.0] * 5
    if n >= 1000:
        assert got[-6:-1].tolist() == [0.0] * 5 and float(got[-1]) > 0.0 and got[500:504].tolist() == [0.0] * 4 and int((got > 0).sum()) > 900


# ------------------------------------------------------------------------------------------------------------------ depth_loss
def _loss_inputs(n, valid, dev):
    g = torch.Generator().manual_seed(300 + n)
    zc, zf = 1.0 + 7.0 * torch.rand(n, generator=g), 1.0 + 7.0 * torch.rand(n, generator=g)
    d = 1.0 + 7.0 * torch.rand(n, generator=g)
    if valid != "all":
        junk = torch.tensor([0.0, -2.0, float("nan"), float("inf"), -float("inf")])
        d = junk[torch.arange(n) % 5].clone()
        if valid == "one":
            d[n // 2] = 3.25
    return zc, zf, d


@pytest.mark.parametrize("with_f", [True, False])
@pytest.mark.parametrize("valid", ["none", "one", "all"])
@pytest.mark.parametrize("n", [1, 5, 1000, 8453])
def test_depth_loss_against_fp64(gpu_device, n, valid, with_f):
    ops = _ops()
    zc, zf, d = _loss_inputs(n, valid, gpu_device)
    weight, near, far = 0.37, 1.0, 8.0
    v_ref, m_ref, nv, dc_ref, df_ref = Z.loss64(zc, zf if with_f else None, d, near, far, weight)
    assert nv == {"none": 0, "one": 1, "all": n}[valid]
    dev = lambda t: t.to(gpu_device)
    args = (dev(zc), dev(zf) if with_f else None, dev(d), near, far, weight)
    out, d_c, d_f = ops.depth_loss(*args)
    out2, d_c2, d_f2 = ops.depth_loss(*args)
    torch.cuda.synchronize()
    e_v = abs(float(out[0]) - v_ref)
    print(f"[depth_loss n = {n}, valid {valid}, zexp_f {with_f}] value error {e_v:.2e} of {v_ref:.4f}")
    assert out.shape == (3,) and e_v <= 2e-6 * max(1.0, abs(v_ref))
    assert abs(float(out[1]) - m_ref) <= 2e-6 * max(1.0, m_ref) and float(out[2]) == float(nv)
    bad = ~(torch.isfinite(d) & (d > 0))
    for got, ref, key in ((d_c, dc_ref, "d_c"), (d_f, df_ref, "d_f")):
        if got is None:
            assert key == "d_f" and not with_f
            continue
        assert bool(torch.isfinite(got).all())
        assert float((got.cpu().double() - ref).abs().max()) <= 2e-6 * float(ref.abs().max()) + 1e-30
        assert float(got.cpu()[bad].abs().sum()) == 0.0                      # exactly zero where there is no measurement
    if valid == "none":
        assert float(out[0]) == 0.0 and float(out[1]) == 0.0 and float(d_c.abs().max()) == 0.0 and (d_f is None or float(d_f.abs().max()) == 0.0)
    assert torch.equal(out, out2) and torch.equal(d_c, d_c2) and (d_f is None or torch.equal(d_f, d_f2))
    assert int(out.storage_offset()) == 0 and int(out._base.view(torch.int32)[3].item()) == 0          # the arrival counter is zero again
    # a second call on the SAME buffer (counter words as the first call left them) gives the same bits
    from mc_nerf_amd import _geo
    buf = out._base.clone()
    d_c3 = torch.empty_like(d_c)
    d_f3 = torch.empty_like(d_f) if d_f is not None else None
    _geo.call(LOSS, args[0], args[1], args[2], n, near, 1.0 / (far - near), weight, buf, d_c3, d_f3, ops._stream())
    assert torch.equal(buf[:3], out) and torch.equal(d_c3, d_c) and int(buf.view(torch.int32)[3].item()) == 0


def test_depth_loss_fn_scales_by_the_upstream_gradient(gpu_device):
    from mc_nerf_amd.model.render import DepthLossFn
    g = torch.Generator().manual_seed(5)
    zc, zf, d = (1.0 + 7.0 * torch.rand(300, generator=g) for _ in range(3))
    d[::3] = 0.0                                                              # a third of the rays has no measurement
    ok = d > 0
    zc, zf, d = zc.to(gpu_device), zf.to(gpu_device), d.to(gpu_device)
    fc, ff = zc.clone().requires_grad_(True), zf.clone().requires_grad_(True)
    (3.0 * DepthLossFn.apply(fc, ff, d, 1.0, 8.0, 0.5)).backward()
    rc, rf = zc.double().requires_grad_(True), zf.double().requires_grad_(True)
    okd = ok.to(gpu_device)
    term = lambda r: ((((r - d.double()) / 7.0) ** 2) * okd).sum() / int(ok.sum())
    (3.0 * 0.5 * (term(rc) + term(rf))).backward()
    assert float((fc.grad.double() - rc.grad).abs().max()) <= 2e-6 * float(rc.grad.abs().max())
    assert float((ff.grad.double() - rf.grad).abs().max()) <= 2e-6 * float(rf.grad.abs().max())
    assert float(fc.grad[~okd].abs().sum()) == 0.0
    fc2 = zc.clone().requires_grad_(True)
    DepthLossFn.apply(fc2, None, d, 1.0, 8.0, 0.5).backward()
    assert fc2.grad is not None and float((fc2.grad.double() - rc.grad / 3.0).abs().max()) <= 2e-6 * float(rc.grad.abs().max())
    empty = torch.zeros(0, device=gpu_device, requires_grad=True)
    assert float(DepthLossFn.apply(empty, None, torch.zeros(0, device=gpu_device), 1.0, 8.0, 0.5)) == 0.0
    none = zc.clone().requires_grad_(True)                                    # no valid target: an exact zero, exact-zero gradients
    v = DepthLossFn.apply(none, None, torch.zeros_like(d), 1.0, 8.0, 0.5)
    v.backward()
    assert float(v) == 0.0 and float(none.grad.abs().max()) == 0.0
