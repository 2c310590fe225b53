"""composite_fwd_kernel / composite_bwd_kernel (csrc/composite.hip) against the fp64 restatement of tests/composite_ref.py, on the
cases of its table (the same inputs tests/test_composite_ref_cpu.py runs through the fp32 oracle), at the bars of
test_a_ops_gpu.py::test_composite_fwd_bwd -- composite_ref.TOL, absolute.  One line per case with the measured errors is printed.

  every case       all outputs of the fullest call (eps_sel, depth, jitter as the case has it) and the backward against the reference;
                   wmax_bits == max(w_sel) and gmax_bits == max |d_sig_rgb| of the device outputs EXACTLY (a maximum does not round);
  chunk edges      S = 2, 3, 63, 64, 65, 127, 129, 160 at 53 rays: dead lanes, one sample over a 64-lane chunk, one under;
  flag matrix      white_back x eps_sel x want_depth x jitter at S = 65: what a setting produces is right AND the bits of the fullest call
                   (computing depth or selection weights must not change rgb); backward at both white_back values;
  grid-stride      8192 + 261 rays: the waves of blocks 0 .. 65 walk two rays.  Rendering is per ray, so the kernel called on the slices
                   [8192:] and [4000:4007] must give the bits of those rows of the full call -- a carry or an LDS word left over from the
                   ray a wave handled before would show; both running maxima are planted in second-round rays;
  large LDS        S = 640 (51 200 B, under the 64 KiB switch), 1024 (81 920 B), 2048 (163 840 B: the bound of mcnerf_composite_bwd);
  refusals         the backward at S = 2049 is refused by the argument check; N = 0 returns empty outputs; N = 1 is a case of the table.

Measured on MI355X, largest error over the cases (bar): S <= 160 and the 8453-ray case: rgb 2.5e-7 (2e-6), depth 7.9e-7 (2e-5), opacity
2.4e-7 (2e-6), w_sel 1.7e-7 (2e-6), d_sig_rgb 5.6e-7 (5e-6).  S = 640 / 1024 / 2048: rgb 3.1e-7, w_sel 1.8e-7, d_sig_rgb 4.1e-7, and depth
1.7e-6 / 3.8e-6 / 4.1e-6, opacity 7.2e-7 / 1.6e-6 / 1.9e-6: the error of the depth pass grows with S (1 - expf(-sd) of ever smaller sd
keeps an absolute 6e-8 per sample, summed over the samples that carry weight) and at S = 2048 opacity sits just under its bar."""
import pytest
import torch

import composite_ref as R

pytestmark = pytest.mark.gpu

_CACHE = {}


def _ops():
    from mc_nerf_amd import ops
    return ops


def _case(name, dev):
    """(host inputs, fp64 reference, device inputs) of a table case: made once, shared, never written to."""
    if name not in _CACHE:
        inp = R.make(name)
        _CACHE[name] = (inp, R.reference(inp), {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()})
    return _CACHE[name]


def _rows_of(d, sl):
    """The device inputs of the rays `sl` alone (contiguous copies)."""
    cut = lambda t: t[sl].contiguous()
    return dict(sig_rgb=cut(d["sig_rgb"]), rays_d=cut(d["rays_d"]), z=cut(d["z"]) if d["z"].dim() == 2 else d["z"],
                jitter=None if d["jitter"] is None else cut(d["jitter"]), eps=cut(d["eps"]), eps_sel=cut(d["eps_sel"]),
                d_rgb=cut(d["d_rgb"]), white_back=d["white_back"])


def _run(d, eps_sel=True, want_depth=True, backward=True, d_rgb=None):
    """Both kernels on device inputs -> dict(rgb, depth, opacity, w_sel, wmax, d_sig_rgb, gmax); what a setting does not produce is None."""
    ops = _ops()
    grid, rows = (None, d["z"]) if d["z"].dim() == 2 else (d["z"], None)
    rgb, depth, opac, w_sel, wmax = ops.composite_fwd(d["sig_rgb"], d["rays_d"], grid, d["jitter"], d["eps"], d["eps_sel"] if eps_sel else None,
                                                      d["white_back"], want_depth, z_rows=rows)
    out = dict(rgb=rgb, depth=depth, opacity=opac, w_sel=w_sel, wmax=wmax, d_sig_rgb=None, gmax=None)
    if backward:
        out["d_sig_rgb"], out["gmax"] = ops.composite_bwd(d["sig_rgb"], grid, d["jitter"], d["eps"], d["d_rgb"] if d_rgb is None else d_rgb,
                                                          d["white_back"], True, z_rows=rows)
    torch.cuda.synchronize()
    return out


def _maxima_exact(label, out):
    if out["w_sel"] is not None:
        wmax, top = float(out["wmax"].view(torch.float32).item()), float(out["w_sel"].max())
        assert wmax == top, f"[{label}] wmax_bits holds {wmax!r}, the largest w_sel written is {top!r}"
    if out["d_sig_rgb"] is not None:
        gmax, g = float(out["gmax"].view(torch.float32).item()), out["d_sig_rgb"].abs()
        k = torch.unravel_index(g.reshape(-1).argmax(), g.shape)
        assert gmax == float(g.max()), (f"[{label}] gmax_bits holds {gmax!r}, the largest |d_sig_rgb| written is {float(g.max())!r} "
                                        f"(ray {int(k[0])}, sample {int(k[1])}, component {int(k[2])})")


def _check(label, out, ref):
    errs, bad = R.compare(label, out, ref)
    print(R.line(label, errs))
    assert not bad, "\n".join(bad)
    _maxima_exact(label, out)
    return errs


def _same_bits(label, got, want, keys=R.OUTPUTS):
    for k in keys:
        if got[k] is None:
            continue
        a, b = got[k].contiguous().view(torch.int32), want[k].contiguous().view(torch.int32)
        if not torch.equal(a, b):
            ne = (a != b).reshape(a.shape[0], -1)
            ray = int(ne.any(dim=1).nonzero()[0])
            col = int(ne[ray].nonzero()[0])
            raise AssertionError(f"[{label}] {k}: {int(ne.sum())} words differ, the first in ray {ray} at "
                                 f"{'sample ' + str(col // (4 if k == 'd_sig_rgb' else 1)) if k in ('w_sel', 'd_sig_rgb') else 'component ' + str(col)}: "
                                 f"{float(got[k].reshape(a.shape[0], -1)[ray, col])!r} != {float(want[k].reshape(a.shape[0], -1)[ray, col])!r}")


@pytest.mark.parametrize("name", [n for n in R.CASES if n != "stride"])
def test_matches_the_fp64_reference(gpu_device, name):
    _, ref, d = _case(name, gpu_device)
    _check(name, _run(d), ref)


@pytest.mark.parametrize("jitter", [True, False])
@pytest.mark.parametrize("want_depth", [True, False])
@pytest.mark.parametrize("eps_sel", [True, False])
@pytest.mark.parametrize("white_back", [True, False])
def test_flag_matrix(gpu_device, white_back, eps_sel, want_depth, jitter):
    name = f"flags_wb{int(white_back)}_jit{int(jitter)}"
    inp, ref, d = _case(name, gpu_device)
    assert d["white_back"] == white_back and (d["jitter"] is not None) == jitter
    full = _run(d)
    out = _run(d, eps_sel=eps_sel, want_depth=want_depth)
    label = f"{name}, eps_sel {'given' if eps_sel else 'None'}, depth {'wanted' if want_depth else 'off'}"
    assert (out["w_sel"] is not None) == eps_sel and (out["wmax"] is not None) == eps_sel
    assert (out["depth"] is not None) == want_depth and (out["opacity"] is not None) == want_depth
    assert out["rgb"] is not None and out["d_sig_rgb"] is not None
    _check(label, out, ref)
    _same_bits(label + " against the fullest call", out, full)
    # depth, opacity and the selection weights do not depend on white_back: the bits of the other setting's call
    other = _run(_case(f"flags_wb{int(not white_back)}_jit{int(jitter)}", gpu_device)[2], backward=False)
    _same_bits(label + " against the other white_back", out, other, keys=("depth", "opacity", "w_sel"))


def test_grid_stride(gpu_device):
    inp, ref, d = _case("stride", gpu_device)
    G = R.GRID_WAVES
    assert inp["sig_rgb"].shape[0] == G + 261
    full = _run(d)
    _check("stride", full, ref)
    # both maxima sit in rays that are the SECOND of their waves, and nothing in the first round reaches them
    w, g = full["w_sel"], full["d_sig_rgb"].abs()
    assert float(w[:G].max()) < float(w[G:].max()) == float(w[R.W_PLANT].max())
    assert float(g[:G].max()) < float(g[G:].max()) == float(g[R.G_PLANT, :, 0].max())
    assert float(full["wmax"].view(torch.float32).item()) == float(w[R.W_PLANT].max())
    assert float(full["gmax"].view(torch.float32).item()) == float(g[R.G_PLANT, :, 0].max())
    # two identical calls: the same bits
    _same_bits("stride, repeated", _run(d), full)
    # per ray: a call on a slice gives the bits of those rows of the full call
    for sl in (slice(G, None), slice(4000, 4007)):
        part = _run(_rows_of(d, sl))
        label = f"stride, rays [{sl.start}:{'' if sl.stop is None else sl.stop}] alone"
        _same_bits(label, part, {k: (None if full[k] is None else full[k][sl]) for k in R.OUTPUTS})
        _maxima_exact(label, part)


@pytest.mark.parametrize("name", ["edge_S129_rows", "stride"])
def test_zero_upstream_gradient(gpu_device, name):
    _, _, d = _case(name, gpu_device)
    out = _run(d, d_rgb=torch.zeros_like(d["d_rgb"]))
    assert int(torch.count_nonzero(out["d_sig_rgb"])) == 0
    assert int(out["gmax"].item()) == 0


def test_backward_refuses_more_samples_than_fit_the_lds(gpu_device):
    from mc_nerf_amd._lib import McnerfError
    ops, dev = _ops(), gpu_device
    N, S = 2, 2049                                         # 4 waves x 5 floats x 2049 samples: 20 B over the 160 KiB of a CU
    z = torch.linspace(1, 8, S, device=dev)
    sr, eps, g = torch.zeros(N, S, 4, device=dev), torch.zeros(N, S, device=dev), torch.ones(N, 3, device=dev)
    with pytest.raises(McnerfError, match="invalid argument"):
        ops.composite_bwd(sr, z, None, eps, g, True)
    with pytest.raises(McnerfError, match="invalid argument"):
        ops.composite_bwd(sr, None, None, eps, g, True, z_rows=z.expand(N, S).contiguous())
    torch.cuda.synchronize()                               # refused by the argument check: nothing was launched, nothing is pending


@pytest.mark.parametrize("rows", [False, True])
def test_no_rays(gpu_device, rows):
    ops, dev = _ops(), gpu_device
    S = 65
    e = lambda *shape: torch.empty(*shape, device=dev)
    grid, z_rows = (None, e(0, S)) if rows else (torch.linspace(1, 8, S, device=dev), None)
    rgb, depth, opac, w_sel, wmax = ops.composite_fwd(e(0, S, 4), e(0, 3), grid, e(0), e(0, S), e(0, S), True, True, z_rows=z_rows)
    assert rgb.shape == (0, 3) and depth.shape == (0, 1) and opac.shape == (0, 1) and w_sel.shape == (0, S) and int(wmax.item()) == 0
    dsr, gmax = ops.composite_bwd(e(0, S, 4), grid, e(0), e(0, S), e(0, 3), True, True, z_rows=z_rows)
    assert dsr.shape == (0, S, 4) and int(gmax.item()) == 0
    torch.cuda.synchronize()
