"""tests/encode_ref.py checked without a GPU.

The bars of tests/test_encode_ops_gpu.py (4 units of 2^-24 w_f forward, 8 units of 2^-24 abs_sum backward) are meaningful only if
plain fp32 arithmetic meets them with room to spare: on EVERY case of the shared table fp32 torch (the oracle's formulation and its
autograd) must lie within HALF of each bar of the fp64 restatement.  A case that breaks this gets other inputs, never another bar.
The restatement's backward is checked against fp64 autograd of its own forward formula."""
import math

import pytest
import torch

import encode_ref as R
from oracle import mcnerf_oracle as O


@pytest.fixture(scope="module")
def table():
    """name -> (inputs, fp64 reference), computed once and shared."""
    out = {}
    for name in R.CASES:
        inp = R.make(name)
        out[name] = (inp, R.reference(inp))
    return out


def test_case_table_covers_the_issue():
    c = R.CASES
    got = {(v["F"], v["n"], v["weights"], v["spread"]) for v in c.values()}
    assert got == {(F, n, w, s) for F in (0, 1, 4, 6, 10) for n in (1, 8, 9, 85, 86, 777) for w in (("ones", "mid", "zeros") if F else ("ones",))
                   for s in (7.0, 200.0)}
    assert len({v["seed"] for v in c.values()}) == len(c)
    assert 8 * 30 == 240 and 9 * 30 == 270 and 85 * 3 == 255 and 86 * 3 == 258            # either side of a 256-thread block
    assert c[R.FUSED_CASE] == dict(F=10, n=777, weights="ones", spread=7.0, seed=c[R.FUSED_CASE]["seed"])
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    assert R.PLANTS[:5] == (0.0, -0.0, 1e-30, 3.5, -3.5) and math.copysign(1.0, R.PLANTS[1]) == -1.0
    assert R.PLANTS[5:9] == tuple(f32(k * math.pi / 4) for k in (1, 2, 3, 4)) and R.PLANTS[9:] == tuple(f32(k * math.pi / 4) / 512 for k in (1, 2, 3, 4))


def test_weights_are_as_described():
    for F in R.FREQS:
        assert torch.equal(R.weights("ones", F), torch.ones(F))
        if F == 0:
            continue
        z = R.weights("zeros", F)
        assert float(z[-1]) == 0.0 and int((z == 0).sum()) == F - F // 2 and set(z.tolist()) <= {0.0, 1.0}
        m = R.weights("mid", F)
        assert m.dtype == torch.float32 and int(((m > 0) & (m < 1)).sum()) == 1            # mid-ramp: one partial weight,
        if F >= 4:
            assert float(m[0]) == 1.0 and float(m[-1]) == 0.0                              # ones below it and exact zeros above


def test_inputs_are_as_described(table):
    for name, (inp, _) in table.items():
        c = R.CASES[name]
        x = inp["x"]
        assert x.shape == (c["n"], 3) and inp["barf_w"].shape == (c["F"],) and inp["d_out"].shape == (c["n"], 3 + 6 * c["F"])
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in inp.values())
        k = min(len(R.PLANTS), x.numel())
        assert torch.equal(x.view(-1)[:k].view(torch.int32), torch.tensor(R.PLANTS[:k], dtype=torch.float32).view(torch.int32))
        assert float(x.view(-1)[k:].abs().max() if x.numel() > k else 0.0) <= c["spread"] / 2
        if c["n"] == 777:
            assert float(x.abs().max()) > 0.45 * c["spread"]
        again = R.make(name)
        assert all(torch.equal(inp[k], again[k]) for k in inp)


def test_planted_quarter_turns_land_on_the_boundaries(table):
    """The range reduction rounds to the nearest quarter turn.  The planted values sit within an fp32 rounding of k / 8 turns: for pi/4
    and 3 pi/4 (k odd) the boundary between two quarter turns, where the reduced angle is +-pi/4, the end of the polynomials' interval;
    for pi/2 and pi (k even) the centre of a quarter turn, where the sine or the cosine passes through zero -- at octave 0 directly, at
    octave 9 for the values divided by 2^9."""
    inp, ref = table["F10_n8_ones_x7"]
    x = inp["x"].view(-1)
    for i, q in enumerate((1, 2, 3, 4)):
        for at, f in ((5 + i, 0), (9 + i, 9)):
            turns = float(x[at].double() * 2.0 ** f / (2 * math.pi))
            assert abs(turns - q / 8) < 1e-7, (at, f, turns)
    # sin(pi) and cos(pi / 2) of the fp32 neighbours: tiny, but not zero -- the reference resolves them
    out = ref["out"]
    ch = lambda axis, f, cos: 3 + axis * 20 + (10 if cos else 0) + f
    assert 0 < abs(float(out[2, ch(2, 0, False)])) < 1e-6                          # x[8] = fl32(pi): element 8 = point 2, axis 2
    assert 0 < abs(float(out[2, ch(0, 0, True)])) < 1e-6                           # x[6] = fl32(pi / 2): point 2, axis 0


@pytest.mark.parametrize("name", list(R.CASES))
def test_fp32_torch_within_half_of_every_bar(table, name):
    inp, ref = table[name]
    got = R.torch32(inp)
    units, bad = R.compare(name + ", fp32 torch at half the bars", got, ref, inp["barf_w"], tol_scale=0.5)
    print(R.line(name + ", fp32 torch", units))
    assert not bad, "\n".join(bad)
    # exact zeros where the weight is zero
    zero = R.channel_weights(inp["barf_w"]) == 0
    assert int(torch.count_nonzero(got["out"][:, zero])) == 0 and int(torch.count_nonzero(ref["out"][:, zero])) == 0


def test_bare_fp32_sin_and_cos_are_within_a_unit(table):
    """What the four units of the forward bar are made of: torch's CPU fp32 sin and cos on the arguments of the table."""
    worst = 0.0
    for name, (inp, _) in table.items():
        F = R.CASES[name]["F"]
        if F == 0:
            continue
        arg = inp["x"].unsqueeze(-1) * (2.0 ** torch.arange(F, dtype=torch.float32))
        s, c = R._sincos(inp["x"], F)
        worst = max(worst, float((arg.sin().double() - s).abs().max()) / R.U24, float((arg.cos().double() - c).abs().max()) / R.U24)
    print(f"worst |fp32 sin / cos - fp64| = {worst:.3f} units of 2^-24")
    assert worst <= 1.0


def test_embed32_is_the_oracle(table):
    for name, (inp, _) in table.items():
        c = R.CASES[name]
        if c["F"] == 0 or c["weights"] == "zeros":
            continue
        cfg = O.RenderCfg(n_freqs=c["F"], barf_mode=c["weights"] == "mid", barf_start=R.BARF["barf_start"], barf_end=R.BARF["barf_end"])
        assert torch.equal(R.embed32(inp["x"], inp["barf_w"]), O.embed(inp["x"], R.BARF["step_r"], cfg)), name


def test_reference_backward_is_the_gradient_of_its_forward(table):
    for name in ("F10_n9_mid_x7", "F6_n8_zeros_x200", "F0_n9_ones_x7", "F1_n1_mid_x7"):
        inp, ref = table[name]
        F = R.CASES[name]["F"]
        x = inp["x"].double().clone().requires_grad_(True)
        arg = x.unsqueeze(-1) * (2.0 ** torch.arange(F, dtype=torch.float64))
        w = inp["barf_w"].double()
        out = torch.cat([x, torch.cat([arg.sin() * w, arg.cos() * w], dim=-1).reshape(x.shape[0], 6 * F)], dim=-1)
        assert float((out.detach() - ref["out"]).abs().max()) <= 1e-15
        (out * inp["d_out"].double()).sum().backward()
        assert float((x.grad - ref["d_x"]).abs().max()) <= 1e-12 * float(ref["abs_sum"]["d_x"].max())
        assert bool((ref["abs_sum"]["d_x"] >= ref["d_x"].abs() * (1 - 1e-12)).all())
