"""The device-free part of tests/mlp_edges_ref.py: the restated gradient scale (`grad_scale`) and its recovery from a stored plane
(`recover_scale`), `dw_reference` on synthetic row-major operands against fp64 autograd of a net with two
trunk layers (the second a skip layer) and both heads, and the tile / unit arithmetic the tail-contract checks rest on."""
import math
from types import SimpleNamespace

import numpy as np
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


# ------------------------------------------------------------------------------------------------ the gradient scale and its recovery
def _f32_neighbours(x):
    x = np.float32(x)
    return [float(np.nextafter(x, np.float32(0))), float(x), float(np.nextafter(x, np.float32(np.inf)))]


def test_grad_scale_is_the_whole_device_function():
    """`grad_scale` against mcn16_grad_scale's three branches as csrc/mcnerf_16.h writes them: 1 for a word that is zero, NaN or at /
    above 3e38f, 2^100 for every word below 2^-96 (the smallest denormal included), else the power of two that puts the word into
    (2^3, 2^4] -- at 2^k and at both of its fp32 neighbours, where ceilf(log2f(.)) decides the exponent.  log2f is an fp32 function: just
    above 2^k it returns k until log2(1 + eps) reaches half an ulp of k, so the interval's upper end is 2^4 (1 + 2^-18) (half an ulp of
    |k| < 128 is at most 2^-18; times ln 2), not 2^4 itself, and the exponent steps at the fp32 neighbour only for |k| <= 1."""
    below_limit = float(np.nextafter(np.float32(3e38), np.float32(0)))
    assert [E.grad_scale(v) for v in (0.0, -0.0, float("nan"), float("inf"), 3e38, -1.0)] == [1.0] * 6
    assert E.grad_scale(float(np.float32(3e38))) == 1.0 and E.grad_scale(below_limit) == 2.0 ** -124
    table = [below_limit, 2.0 ** -149]
    for k in (-126, -97, -96, -95, -1, 0, 1, 4, 100, 127):
        table += _f32_neighbours(2.0 ** k)
    for gmax in table:
        sg = E.grad_scale(gmax)
        m, e = math.frexp(sg)
        assert m == 0.5 and sg > 0, (gmax, sg)                      # a power of two
        if gmax >= 2.0 ** -96:
            assert 2.0 ** 3 < gmax * sg <= 2.0 ** 4 * (1 + 2.0 ** -18), (gmax, sg)
        else:
            assert sg == 2.0 ** 100, (gmax, sg)
    # 2^k itself and its lower neighbour take the larger scale; the upper neighbour half of it where fp32 log2f can tell it from 2^k
    for k in (-95, -1, 0, 1, 4, 100):
        lo, at, hi = (E.grad_scale(v) for v in _f32_neighbours(2.0 ** k))
        assert lo == at == 2.0 ** (4 - k) and hi == 2.0 ** ((3 if abs(k) <= 1 else 4) - k), k
    assert E.grad_scale(2.0 ** -96) == E.grad_scale(float(np.nextafter(np.float32(2.0 ** -96), np.float32(1)))) == 2.0 ** 100
    for k in (-95, 4, 100):                                          # ... and a little further up where it cannot: the scale has halved by 2^k (1 + 2^-16)
        assert E.grad_scale(2.0 ** k * (1 + 2.0 ** -16)) == 2.0 ** (3 - k), k
    # fp32 inputs: a double that rounds to 2^0 in fp32 is 2^0
    assert E.grad_scale(1.0 + 2.0 ** -30) == 16.0
    # (the values the callers from before the clamp was restated rely on)
    assert E.grad_scale(1e-4) == 2.0 ** 17 and E.grad_scale(1.0) == 16.0 and E.grad_scale(1.5) == 8.0 and E.grad_scale(4e-4) == 2.0 ** 15


def _synthetic_dsh(mode, col27, tiles):
    """A dsh workspace whose column 27 holds `col27` (fp64, one value per row), built with torch casts in the layouts of
    ops.decode_frags_16: channel 27 = 16 s + 8 (j >> 2) + 4 h + (j & 3) sits at k-step 1, lane half 0, element 7."""
    rows = col27.shape[0]
    if mode == "f32":
        w = torch.zeros(tiles * 32, 32)
        w[:rows, 27] = col27.float()
        return w.reshape(-1)
    dt = torch.bfloat16 if mode == "bf16" else torch.float16
    parts = 2 if mode == "f16x3" else 1
    w = torch.zeros(tiles, parts, 2, 2, 32, 8, dtype=dt)
    v = torch.zeros(tiles * 32, dtype=torch.float64)
    v[:rows] = col27
    hi = v.to(dt)
    w[:, 0, 1, 0, :, 7] = hi.view(tiles, 32)
    if parts == 2:                                                   # mcnx3_split2: lo = f16(v - hi)
        w[:, 1, 1, 0, :, 7] = (v - hi.double()).to(dt).view(tiles, 32)
    w[:, :, 0, 1, :, 3] = 7.0                                        # (channel 7: something that is not column 27)
    return w.reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("mode", E.ALL_MODES)
def test_recover_scale_reads_the_exponent_off_a_stored_plane(mode):
    """`recover_scale` on synthetic planes: the exponent that was put in comes out, over the scales a run can take (2^-124 .. 2^100 times
    a gradient that keeps the product in the 16-bit range), whatever the other columns and rows hold; a scale off by less than a power
    of two, a zero plane (what an f16 plane holds when d_out * 2^100 is below 2^-25: the scale cannot be read there) and a NaN are refused."""
    g = torch.Generator().manual_seed(5)
    rows = 45
    unit = torch.randn(rows, 4, generator=g, dtype=torch.float64).clamp(-1.4, 1.4)
    unit[7, 0] = -1.5                                                # the row the scale is read at; negative on purpose
    for e_out, e_sg in ((0, 3), (-100, 100), (-110, 100), (20, -17), (120, -117), (0, -17)):
        d_out = (unit * 2.0 ** e_out).float()
        e_sg = 0 if mode == "f32" else e_sg
        dsh = _synthetic_dsh(mode, d_out[:, 0].double() * 2.0 ** e_sg, 2)
        assert E.recover_scale(mode, dsh, d_out) == e_sg, (mode, e_out, e_sg)
        assert float(E.sigma_column(mode, dsh, rows)[7]) == pytest.approx(float(d_out[7, 0]) * 2.0 ** e_sg, rel=2.0 ** -8)
    d_out = unit.float()
    for bad in (d_out[:, 0].double() * 12.0, torch.zeros(rows, dtype=torch.float64), d_out[:, 0].double() * float("nan")):
        with pytest.raises(AssertionError):
            E.recover_scale(mode, _synthetic_dsh(mode, bad, 2), d_out)
