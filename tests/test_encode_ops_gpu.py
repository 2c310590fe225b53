"""encode_kernel / encode_bwd_kernel (csrc/select.hip), called through ops.encode / ops.encode_bwd, against the fp64 restatement of
tests/encode_ref.py on the cases of its table (the inputs tests/test_encode_ref_cpu.py runs through fp32 torch), under its bars: forward
4 units of 2^-24 w_f per channel, the pass-through channels bit-exact, channels of a zero weight exactly 0.0; backward 8 units of
2^-24 abs_sum.  One line per case with the worst error in those units is printed.

  every case   F = 0, 1, 4, 6, 10 frequencies x n = 1, 8, 9, 85, 86, 777 points (either side of a 256-thread block in both kernels) x
               weights all ones / mid-ramp / trailing zeros x |x| <= 3.5 and <= 100, with signed zeros, 1e-30, the scene bound and
               quarter-turn boundaries of the range reduction at the first and the top octave planted;
  n = 0        an empty tensor from both;
  fused path   on the F = 10, all-ones, 777-point case the encoding that the fused MLP forward saves (32-wide net) agrees with the
               restatement under TWICE the forward bar: the stand-alone and the fused encodings must not drift apart.

Measured on MI355X, worst over all cases: forward 1.93 units (bar 4), backward 2.97 units (bar 8); the fused path 1.50 units (bar 8)."""
import pytest
import torch

import encode_ref as R
from oracle import mcnerf_oracle as O

pytestmark = pytest.mark.gpu


def _ops():
    from mc_nerf_amd import ops
    return ops


@pytest.mark.parametrize("name", list(R.CASES))
def test_matches_the_fp64_reference(gpu_device, name):
    ops, dev = _ops(), gpu_device
    inp = R.make(name)
    ref = R.reference(inp)
    x, w, g = inp["x"].to(dev), inp["barf_w"].to(dev), inp["d_out"].to(dev)
    got = {"out": ops.encode(x, w), "d_x": ops.encode_bwd(x, w, g)}
    torch.cuda.synchronize()
    units, bad = R.compare(name, got, ref, inp["barf_w"])
    print(R.line(name, units))
    assert not bad, "\n".join(bad)
    zero = R.channel_weights(inp["barf_w"]) == 0
    assert int(torch.count_nonzero(got["out"].cpu()[:, zero])) == 0                # a zero weight: exactly 0.0
    assert torch.equal(ops.encode(x, w), got["out"]) and torch.equal(ops.encode_bwd(x, w, g), got["d_x"])


@pytest.mark.parametrize("F", [0, 10])
def test_no_points(gpu_device, F):
    ops, dev = _ops(), gpu_device
    x, w = torch.empty(0, 3, device=dev), torch.ones(F, device=dev)
    out = ops.encode(x, w)
    d_x = ops.encode_bwd(x, w, torch.empty(0, 3 + 6 * F, device=dev))
    torch.cuda.synchronize()
    assert out.shape == (0, 3 + 6 * F) and d_x.shape == (0, 3)


def test_fused_forward_saves_the_same_encoding(gpu_device):
    """x = rays_o + rays_d * 0 exactly, so the fused forward encodes the points of the case."""
    ops, dev = _ops(), gpu_device
    inp = R.make(R.FUSED_CASE)
    ref = R.reference(inp)
    n = inp["x"].shape[0]
    nc = O.NetCfg(4, 32, (2,))
    net = ops.Net(nc.depth, nc.width, nc.skips[0])
    p = O.init_params(nc, 132)
    flat = ops.flatten_params(net, [p[k].to(dev) for k in net.names()], dev)
    packed = ops.pack_weights(net, flat, precision="f32")
    g = torch.Generator().manual_seed(9)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).to(dev)
    out = torch.empty(n, 1, 4, device=dev)
    save = ops.alloc_save(net, n, dev)
    ops.mlp_fwd(net, flat, packed, inp["x"].to(dev), d, torch.zeros(1, device=dev), None, inp["barf_w"].to(dev), out, save=save, precision="f32")
    torch.cuda.synchronize()
    enc = save.enc.view(save.capacity, 64)[:n, :63]
    # (-0.0 + 0 = +0.0: the pass-through channels are compared as numbers here)
    units, bad = R.compare("fused forward, " + R.FUSED_CASE, {"out": enc}, ref, inp["barf_w"], tol_scale=2.0, exact=False)
    print(R.line("fused forward, " + R.FUSED_CASE, units))
    assert not bad, "\n".join(bad)
    assert torch.equal(enc[:, :3].cpu(), inp["x"] + 0.0)
    alone = ops.encode(inp["x"].to(dev), inp["barf_w"].to(dev))
    assert float((alone - enc).abs().max()) <= 3 * R.TOL["fwd"] * R.U24              # each within its bar of the same reference
