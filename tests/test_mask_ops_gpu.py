"""The extension library's kernels (csrc/mask.hip, include/mcnerf_ext.h) on the GPU.

  parity        front_weight and composite_bwd_front against the fp64 restatement tests/mask_ref.py, on both input families ("a": the
                table's saturated / empty rays; "b": semi-transparent rays, where fg is anywhere in (0, 1) and the d_fg term is live), at
                S = 2, 3, 63, 64, 65, 129 (chunk edges), 1024 (LDS above 64 KiB), 2048 at 5 rays (the bound), one ray, and 8192 + 261 rays
                (grid stride), each in both depth forms and with white_back on and off.  Bar per case and output:
                e_kernel <= 2 e_fp32 + 16 * 2^-24 * max|ref|, e_fp32 the fp32 restatement's own error on that case (mask_ref.bound).
                The backward runs twice: with the case's d_rgb, and with d_rgb = 0 so that the d_fg term stands alone (max|ref| then
                shrinks with the term).  The measured errors go to profiles/mask_parity.txt.
                Measured on MI355X: all 80 variants pass; the semi-transparent rays at S = 1024 / 2048 sit at fg 1.6e-8 .. 2.8e-8 (bars
                1.1e-6 .. 2.2e-6) and d_sig_rgb 6.0e-8 .. 7.8e-8 (bars 2.1e-6 .. 3.5e-6).  (With the core composite's fp32 arithmetic in
                the mask path those 8 variants were at 5e-6 / 1e-5: the device's expf near 1 is biased by -0.10 * 2^-24, which adds
                linearly over a thousand samples of the transmittance product; the mask path is fp64 per sample for that reason.);
  bit identity  composite_bwd_front(d_fg = None) is ops.composite_bwd word for word, d_sig_rgb and the gmax word, on every case of
                composite_ref.CASES: the two libraries' instantiations of the backward's body (csrc/mcnerf_composite.h) are one computation;
  refusals      S = 2049 is refused with the output untouched; bad segment tables are refused;
  gather_alpha  against indexing the uint8 tensor, K = 1 and K = 3 with cameras [2, 0, 2]; ones for 3-channel images;
  mask_loss     n = 1, 255, 256, 257, 32768 + 261, with and without fg_f: value <= 2e-6 max(1, |ref|), gradients <= 2e-6 max|ref|
                against fp64 (the bars of tests/test_color_calib_gpu.py); two runs are torch.equal; the arrival counter is zero afterwards.
"""
import os

import pytest
import torch

import composite_ref as R
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
        inp = M.variant(shape, family, rows, wb)
        _CACHE[key] = (inp, {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()})
    return _CACHE[key]


def _depth_args(d):
    return (None, d["z"]) if d["z"].dim() == 2 else (d["z"], None)


def _record_parity(key, line):
    """profiles/mask_parity.txt: one line per variant, rewritten by every run of the parity test."""
    path = os.path.join(ROOT, "profiles", "mask_parity.txt")
    head = ("# front_weight / composite_bwd_front (csrc/mask.hip) against the fp64 restatement tests/mask_ref.py; max abs error of the kernel\n"
            "# (e_k) beside the fp32 restatement's own (e_32) and the bar 2 e_32 + 16 * 2^-24 max|ref|; bwd0: d_rgb = 0, the d_fg term alone;\n"
            "# written by tests/test_mask_ops_gpu.py::test_parity_against_fp64\n")
    try:
        lines = {}
        if os.path.isfile(path):
            lines = {l.split(":")[0]: l for l in open(path).read().splitlines() if l and not l.startswith("#")}
        lines[key] = f"{key}: {line}"
        with open(path, "w") as f:
            f.write(head + "\n".join(lines[k] for k in sorted(lines)) + "\n")
    except OSError:                     # (a read-only checkout: the figures are still printed)
        pass


@pytest.mark.parametrize("white_back", [True, False])
@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("shape", M.SHAPES)
def test_parity_against_fp64(gpu_device, shape, family, rows, white_back):
    ops = _ops()
    inp, d = _variant(shape, family, rows, white_back, gpu_device)
    grid, zr = _depth_args(d)
    zero = torch.zeros_like(d["d_rgb"])
    fg = ops.front_weight(d["sig_rgb"], grid, d["jitter"], d["eps"], z_rows=zr)
    got = {"fg": fg}
    got["bwd"], gmax = ops.composite_bwd_front(d["sig_rgb"], grid, d["jitter"], d["eps"], d["d_rgb"], d["d_fg"], white_back, True, z_rows=zr)
    got["bwd0"] = ops.composite_bwd_front(d["sig_rgb"], grid, d["jitter"], d["eps"], zero, d["d_fg"], white_back, z_rows=zr)
    torch.cuda.synchronize()
    assert float(gmax.view(torch.float32).item()) == float(got["bwd"].abs().max())          # (a maximum does not round)
    ref, r32 = M.reference(inp), M.restated32(inp)
    ref0, r320 = M.reference(inp, zero.cpu()), M.restated32(inp, zero.cpu())
    rec, bad = [], []
    for name, g, rf, r3 in (("fg", got["fg"], ref["fg"], r32["fg"]), ("bwd", got["bwd"], ref["d_sig_rgb"], r32["d_sig_rgb"]),
                            ("bwd0", got["bwd0"], ref0["d_sig_rgb"], r320["d_sig_rgb"])):
        assert tuple(g.shape) == tuple(rf.shape)
        (e_k, at), (e_32, _) = R.worst(g, rf), R.worst(r3, rf)
        bar = M.bound(e_32, rf)
        rec.append(f"{name} e_k {e_k:.3e} e_32 {e_32:.3e} bar {bar:.3e} max|ref| {float(rf.abs().max()):.3e}")
        if not e_k <= bar:
            bad.append(f"{rec[-1]} at {at}")
    key = f"{shape} {family} {'rows' if rows else 'grid'} wb{int(white_back)}"
    print(f"[mask parity, {key}] " + "; ".join(rec))
    _record_parity(key, "; ".join(rec))
    assert not bad, (key, bad)
    if family == "b" and inp["sig_rgb"].shape[0] == 53 and inp["sig_rgb"].shape[1] >= 3:
        assert M.semi_transparent_share(fg.cpu()) >= M.FRACTION
        assert float(ref0["d_sig_rgb"].abs().max()) > 1e-3              # the d_fg term is live on these rays


@pytest.mark.parametrize("name", list(R.CASES))
def test_without_d_fg_the_backward_is_the_core_kernels_bits(gpu_device, name):
    ops = _ops()
    inp = R.make(name)
    d = {k: (v.to(gpu_device) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    grid, zr = _depth_args(d)
    core, core_g = ops.composite_bwd(d["sig_rgb"], grid, d["jitter"], d["eps"], d["d_rgb"], d["white_back"], True, z_rows=zr)
    ext, ext_g = ops.composite_bwd_front(d["sig_rgb"], grid, d["jitter"], d["eps"], d["d_rgb"], None, d["white_back"], True, z_rows=zr)
    torch.cuda.synchronize()
    assert torch.equal(ext.view(torch.int32), core.view(torch.int32)), (name, int((ext.view(torch.int32) != core.view(torch.int32)).sum()))
    assert torch.equal(ext_g, core_g) and int(core_g.item()) != 0


def test_refusals_leave_the_output_untouched(gpu_device):
    from mc_nerf_amd import _ext
    from mc_nerf_amd._lib import McnerfError
    ops = _ops()
    N, S = 2, 2049
    sig, eps = torch.zeros(N, S, 4, device=gpu_device), torch.zeros(N, S, device=gpu_device)
    z, d_rgb, d_fg = torch.linspace(1, 8, S, device=gpu_device), torch.ones(N, 3, device=gpu_device), torch.ones(N, device=gpu_device)
    out = torch.full((N, S, 4), 7.0, device=gpu_device)
    with pytest.raises(McnerfError, match="mcnerf_ext_composite_bwd_front.*invalid argument"):
        _ext.call("mcnerf_ext_composite_bwd_front", sig, z, 0, None, eps, d_rgb, d_fg, N, S, 1, out, None, ops._stream())
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    assert ops.front_weight(sig, z, None, eps).shape == (N,)              # (the forward has no LDS bound)
    e = torch.zeros(0, 8, 4, device=gpu_device)                              # N = 0: empty results
    assert ops.front_weight(e, z[:8].contiguous(), None, e[..., 0].contiguous()).shape == (0,)
    assert ops.composite_bwd_front(e, z[:8].contiguous(), None, e[..., 0].contiguous(), e[:, 0, :3].contiguous(), e[:, 0, 0].contiguous()).shape == (0, 8, 4)


# ------------------------------------------------------------------------------------------------------------------ gather_alpha
# b / 255 correctly rounded to fp32 for every byte (torch's own division by a scalar on the device multiplies by a rounded 1 / 255)
BYTE_OVER_255 = torch.tensor([b / 255 for b in range(256)], dtype=torch.float64).float()


@pytest.fixture(scope="module")
def images(gpu_device):
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, 256, (3, 37 * 29, 4), dtype=torch.uint8, generator=g).to(gpu_device)


@pytest.mark.parametrize("cams, seg", [([1], [0, 301]), ([2, 0, 2], [0, 100, 100, 301]), ([2, 0, 2], [0, 101, 201, 301])])
def test_gather_alpha_is_the_indexed_byte(gpu_device, images, cams, seg):
    ops = _ops()
    g = torch.Generator().manual_seed(12)
    pix = torch.randint(0, images.shape[1], (seg[-1],), generator=g).to(gpu_device)
    pix[0], pix[-1] = 0, images.shape[1] - 1
    a = ops.gather_alpha(images, cams, seg, pix)
    cam_of = torch.cat([torch.full((hi - lo,), c, dtype=torch.int64) for c, lo, hi in zip(cams, seg, seg[1:])]).to(gpu_device)
    want = BYTE_OVER_255.to(gpu_device)[images[cam_of, pix, 3].long()]
    assert a.dtype == torch.float32 and torch.equal(a, want)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    ones = ops.gather_alpha(images[..., :3].contiguous(), cams, seg, pix)
    assert torch.equal(ones, torch.ones_like(ones))


def test_gather_alpha_refuses_bad_tables_and_marks_bad_pixels(gpu_device, images):
    from mc_nerf_amd._lib import McnerfError
    ops = _ops()
    pix = torch.zeros(10, dtype=torch.int64, device=gpu_device)
    for cams, seg in (([3], [0, 10]), ([-1], [0, 10]), ([0, 1], [0, 6, 5]), ([0], [1, 10]), ([0] * 65, list(range(66)))):
        with pytest.raises(McnerfError):
            ops.gather_alpha(images, cams, seg, pix if seg[-1] == 10 else torch.zeros(seg[-1], dtype=torch.int64, device=gpu_device))
    with pytest.raises(McnerfError):
        ops.gather_alpha(images, [0], [0, 10, 10], pix)                      # seg_start longer than the cameras + 1
    pix[3], pix[7] = images.shape[1], -1                                     # an id outside the image reads nothing: NaN
    a = ops.gather_alpha(images, [1], [0, 10], pix)
    assert torch.isnan(a).nonzero().flatten().tolist() == [3, 7]


# ------------------------------------------------------------------------------------------------------------------ mask_loss
@pytest.mark.parametrize("with_f", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 32768 + 261])
def test_mask_loss_against_fp64(gpu_device, n, with_f):
    ops = _ops()
    g = torch.Generator().manual_seed(100 + n)
    fg_c, fg_f, a = torch.rand(n, generator=g) * 1.0001, torch.rand(n, generator=g), (torch.randint(0, 256, (n,), generator=g).float() / 255.0)
    weight = 0.37
    m = ((fg_c.double() - a.double()) ** 2).mean() + (((fg_f.double() - a.double()) ** 2).mean() if with_f else 0.0)
    ref = {"value": weight * m, "d_c": 2.0 * weight / n * (fg_c.double() - a.double()), "d_f": 2.0 * weight / n * (fg_f.double() - a.double())}
    dev = lambda t: t.to(gpu_device)
    args = (dev(fg_c), dev(fg_f) if with_f else None, dev(a), weight)
    out, d_c, d_f = ops.mask_loss(*args)
    out2, d_c2, d_f2 = ops.mask_loss(*args)
    torch.cuda.synchronize()
    e_v = abs(float(out[0]) - float(ref["value"]))
    print(f"[mask_loss n = {n}, fg_f {with_f}] value error {e_v:.2e} of {float(ref['value']):.4f}")
    assert e_v <= 2e-6 * max(1.0, abs(float(ref["value"])))
    assert abs(float(out[1]) - float(m)) <= 2e-6 * max(1.0, float(m))
    for got, key in ((d_c, "d_c"), (d_f, "d_f")):
        if got is None:
            assert key == "d_f" and not with_f
            continue
        assert float((got.cpu().double() - ref[key]).abs().max()) <= 2e-6 * float(ref[key].abs().max()) + 1e-30
    assert torch.equal(out, out2) and torch.equal(d_c, d_c2) and (d_f is None or torch.equal(d_f, d_f2))
    assert int(out.storage_offset()) == 0 and int(out._base.view(torch.int32)[3].item()) == 0          # the arrival counter is zero again


def test_mask_loss_fn_scales_by_the_upstream_gradient(gpu_device):
    from mc_nerf_amd.model.render import MaskLossFn
    g = torch.Generator().manual_seed(5)
    fg_c, fg_f, a = (torch.rand(300, generator=g).to(gpu_device) for _ in range(3))
    fc, ff = fg_c.clone().requires_grad_(True), fg_f.clone().requires_grad_(True)
    (3.0 * MaskLossFn.apply(fc, ff, a, 0.5)).backward()
    rc, rf = fg_c.double().requires_grad_(True), fg_f.double().requires_grad_(True)
    (3.0 * 0.5 * (((rc - a.double()) ** 2).mean() + ((rf - a.double()) ** 2).mean())).backward()
    assert float((fc.grad.double() - rc.grad).abs().max()) <= 2e-6 * float(rc.grad.abs().max())
    assert float((ff.grad.double() - rf.grad).abs().max()) <= 2e-6 * float(rf.grad.abs().max())
    fc2 = fg_c.clone().requires_grad_(True)
    MaskLossFn.apply(fc2, None, a, 0.5).backward()
    assert fc2.grad is not None and float((fc2.grad.double() - rc.grad / 3.0).abs().max()) <= 2e-6 * float(rc.grad.abs().max())
    empty = torch.zeros(0, device=gpu_device, requires_grad=True)
    assert float(MaskLossFn.apply(empty, None, torch.zeros(0, device=gpu_device), 0.5)) == 0.0
