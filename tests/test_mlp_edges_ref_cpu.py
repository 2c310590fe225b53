"""The device-free part of tests/mlp_edges_ref.py: `dw_reference` on synthetic row-major operands against fp64 autograd of a net with two
trunk layers (the second a skip layer) and both heads, and the tile / unit arithmetic the tail-contract checks rest on."""
from types import SimpleNamespace

import pytest
import torch

import mlp_edges_ref as E


def test_dw_reference_is_autograd_of_a_two_layer_net():
    D, skip, W, rows = 2, 1, 8, 37
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    shapes = {"xyz_encoding_1.0": (W, 63), "xyz_encoding_2.0": (W, W + 63), "sigma.0": (W, W), "sigma.2": (1, W), "sh.0": (W, W), "sh.2": (27, W)}
    p = {}
    for k, (n, m) in shapes.items():
        p[k + ".weight"], p[k + ".bias"] = (rnd(n, m) / m ** 0.5).requires_grad_(True), rnd(n).requires_grad_(True)
    lin = lambda x, k: torch.nn.functional.linear(x, p[k + ".weight"], p[k + ".bias"])
    pre = []

    def relu(y):
        y.retain_grad()
        pre.append(y)
        return torch.relu(y)
    enc = rnd(rows, 63)
    h0 = relu(lin(enc, "xyz_encoding_1.0"))
    h1 = relu(lin(torch.cat([enc, h0], 1), "xyz_encoding_2.0"))     # the skip layer: [encoding, hidden], model/net_block.py:70-71
    hs = relu(lin(h1, "sigma.0"))
    hc = relu(lin(h1, "sh.0"))
    sigma, sh = lin(hs, "sigma.2"), lin(hc, "sh.2")
    g_sigma, g_sh = rnd(rows, 1), rnd(rows, 27)
    ((sigma * g_sigma).sum() + (sh * g_sh).sum()).backward()

    act = [h.detach() for h in (h0, h1, hs, hc)]                     # slots 0 .. D - 1, D (sigma hidden), D + 1 (sh hidden)
    dy = [y.grad for y in pre]
    assert all(bool((a > 0).any()) and bool((a == 0).any()) for a in act), "every layer needs both ReLU branches"
    dsh = torch.zeros(rows, 32, dtype=torch.float64)
    dsh[:, :27], dsh[:, 27:28] = g_sh, g_sigma                       # column 27 carries d sigma
    ref = E.dw_reference(D, skip, SimpleNamespace(enc=enc, dsh=dsh, act=lambda l: act[l], dy=lambda l: dy[l]))
    assert sorted(ref) == sorted(p)
    for name, t in p.items():
        assert ref[name].shape == t.grad.shape, name
        assert float((ref[name] - t.grad).abs().max()) <= 1e-12 * max(1.0, float(t.grad.abs().max())), name


def test_dw_reference_takes_only_the_rows_it_is_given():
    """A row of NaN behind the operands' last row must not matter: the reference is over the rows handed to it, nothing else."""
    D, W, rows = 1, 4, 5
    g = torch.Generator().manual_seed(1)
    full = lambda *s: torch.cat([torch.randn(rows, *s, generator=g, dtype=torch.float64), torch.full((1, *s), float("nan"), dtype=torch.float64)])
    enc, dsh, act, dy = full(63), full(32), [full(W) for _ in range(D + 2)], [full(W) for _ in range(D + 2)]
    cut = SimpleNamespace(enc=enc[:rows], dsh=dsh[:rows], act=lambda l: act[l][:rows], dy=lambda l: dy[l][:rows])
    ref = E.dw_reference(D, 0, cut)
    assert len(ref) == 2 * D + 8 and all(bool(torch.isfinite(v).all()) for v in ref.values())
    assert torch.equal(ref["sigma.2.bias"], dsh[:rows, 27:28].sum(0))


@pytest.mark.parametrize("R", [128, 256])
def test_covered_tiles(R):
    w = R // 32
    assert E.covered_tiles(0, R) == 0
    assert [E.covered_tiles(n, R) for n in (1, 31, 32, 33, R - 1, R)] == [w] * 6
    assert [E.covered_tiles(n, R) for n in (R + 1, 2 * R, 2 * R + 1)] == [2 * w, 2 * w, 3 * w]
    for rows in range(1, 4 * R + 2):
        t = E.covered_tiles(rows, R)
        assert 32 * t >= rows and 32 * (t - w) < rows and t % w == 0


def test_units():
    assert E.cap_units("f32", 577) == 577 and E.cap_units("f32", 0) == 1                # (ops.alloc_save allocates at least one row)
    for mode in ("f16x3", "f16", "bf16"):
        assert [E.cap_units(mode, n) for n in (0, 1, 256, 257, 320, 576)] == [8, 8, 8, 16, 16, 24]
        for R in (128, 256):                                                            # the passes of a launch stay inside the allocation
            assert all(E.covered_tiles(rows, R) <= E.cap_units(mode, rows) for rows in range(1, 1100))
    assert E.covered_units("f32", 17, 64) == 17 and E.covered_units("f16", 17, 256) == 8 and E.covered_units("f16x3", 129, 128) == 8
    assert E.unit_rows("f32") == 1 and E.unit_rows("bf16") == 32
    assert E.pass_rows("f16x3", 64) == 256 and E.pass_rows("f16x3", 256) == 128 and E.pass_rows("bf16", 64) == 256


def test_unit_bytes_and_tile_planes():
    """`unit_bytes` splits a buffer [slots][units][...]; `tile_planes` shows both planes of an f16x3 tile as stored."""
    buf = torch.arange(2 * 8 * 64, dtype=torch.int32)
    u = E.unit_bytes("f16", buf, 2, 200)                     # 200 rows: 8 tiles per slot
    assert tuple(u.shape) == (2, 8, 256) and torch.equal(u[1, 3].view(torch.int32), buf.view(2, 8, 64)[1, 3])
    W, tiles = 32, 8
    x = torch.zeros(1, tiles, 2, W // 16, 2, 32, 8, dtype=torch.float16)
    x[0, 5, 0, 1, 0, 7, 3], x[0, 5, 1, 1, 0, 7, 3] = 1.0, -1.0          # hi + lo = 0, neither plane is zero
    t = E.tile_planes("f16x3", x.reshape(-1).view(torch.uint8), 1, W, 5)
    assert tuple(t.shape) == (1, 2, 2, 2, 32, 8) and int((t != 0).sum()) == 2 and float(t.sum()) == 0.0
    assert bool((t[..., 8:, :] == 0).all()) and not bool((t[..., 7:, :] == 0).all())
    assert E.grad_scale(1e-4) == 2.0 ** 17 and E.grad_scale(1.0) == 16.0 and E.grad_scale(1.5) == 8.0
