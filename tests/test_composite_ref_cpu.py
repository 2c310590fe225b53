"""tests/composite_ref.py checked without a GPU.

The bars of tests/test_composite_gpu.py (composite_ref.TOL) are meaningful only if plain fp32 arithmetic meets them with room to
spare: for EVERY case of the shared table the fp32 oracle (O.composite, O.sigma2weights, fp32 autograd) must lie within HALF of each
bar of the fp64 restatement.  A case that breaks this gets other inputs, never another bar.  The restatement's gradient is also checked
against central differences of its own forward, so that it rests on more than autograd of itself."""
import pytest
import torch

import composite_ref as R


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
    for S in (2, 3, 63, 64, 65, 127, 129, 160):
        for form in ("grid", "rows"):
            assert c[f"edge_S{S}_{form}"]["N"] == 53 and c[f"edge_S{S}_{form}"]["S"] == S
    assert {(c[k]["white_back"], c[k]["jitter"]) for k in c if k.startswith("flags_")} == {(a, b) for a in (True, False) for b in (True, False)}
    assert all(c[k]["N"] == 53 and c[k]["S"] == 65 and c[k]["rows"] for k in c if k.startswith("flags_"))
    s = c["stride"]
    assert s["N"] == 8192 + 261 and s["S"] == 65 and s["rows"] and not s["white_back"]
    assert [(c[f"lds_S{S}_grid"]["N"], c[f"lds_S{S}_rows"]["N"]) for S in (640, 1024, 2048)] == [(53, 53), (53, 53), (5, 5)]
    assert 4 * 5 * 640 * 4 == 51200 and 4 * 5 * 1024 * 4 == 81920 and 4 * 5 * 2048 * 4 == 163840 == 160 * 1024
    assert c["one_ray"]["N"] == 1


def test_inputs_are_as_described(table):
    for name, (inp, _) in table.items():
        c = R.CASES[name]
        N, S = c["N"], c["S"]
        assert inp["sig_rgb"].shape == (N, S, 4) and inp["rays_d"].shape == (N, 3) and inp["eps"].shape == inp["eps_sel"].shape == (N, S)
        assert all(t.dtype == torch.float32 for t in inp.values() if isinstance(t, torch.Tensor))
        rl = inp["rays_d"].norm(dim=-1)
        assert float(rl.min()) >= 0.5 - 1e-6 and float(rl.max()) <= 1.5 + 1e-6
        assert (inp["jitter"] is None) == (not c["jitter"])
        z = R.depths(inp["z"], inp["jitter"], N)
        delta = z[:, 1:] - z[:, :-1]
        assert bool((delta >= 0).all()), name                                    # sorted
        if c["rows"]:
            assert inp["z"].shape == (N, S)
            dup = (delta == 0).sum(dim=1)
            keep = torch.ones(N, dtype=torch.bool)
            if c["maxima"]:
                keep[[R.W_PLANT, R.G_PLANT]] = False                             # (their rows were rewritten)
            assert bool((dup[keep] >= 1).all()), name                            # a duplicated depth in every ray
        else:
            assert torch.equal(inp["z"], torch.linspace(1, 8, S))
        again = R.make(name)
        assert all(torch.equal(inp[k], again[k]) for k in inp if isinstance(inp[k], torch.Tensor))


def test_planted_rays_do_what_they_are_for(table):
    inp, ref = table["flags_wb1_jit1"]                   # N = 53: empty 0..3, opaque 4..7, saturated 8..9, last 10
    assert float(ref["w_sel"][:4, :-1].max()) < 1e-6                             # empty: nothing before the last sample
    assert float(ref["w_sel"][4:8, 65 // 2:].max()) < 1e-6                       # opaque early: nothing behind the first half
    assert float(inp["sig_rgb"][8:10, :, 0].min() + inp["eps"][8:10].min()) > 20.0      # the x > 20 branch of softplus
    z = R.depths(inp["z"], inp["jitter"], 53).double()
    a_last = 1.0 - torch.exp(-1e10 * torch.nn.functional.softplus(inp["sig_rgb"][10, -1, 0].double() + inp["eps"][10, -1].double()))
    assert 0.05 < float(a_last) < 0.95 and z.shape == (53, 65)                   # the last sample's alpha: far from 0 and from 1
    # saturated over a large delta: u = 1e-10 and an underflowing transmittance (S = 2: delta = 7)
    inp2, ref2 = table["edge_S2_grid"]
    assert float(inp2["sig_rgb"][8, 0, 0]) == 30.0 and float(ref2["w_sel"][8, 1]) < 2e-10


def test_stride_case_plants_both_maxima_behind_the_first_round(table):
    inp, ref = table["stride"]
    G = R.GRID_WAVES
    w = ref["w_sel"]
    assert float(w[:G].max()) < float(w[G:].max()) and float(w[R.W_PLANT, 0]) == float(w.max())
    g = ref["d_sig_rgb"].abs()
    assert float(g[:G].max()) < float(g[G:].max())
    k = torch.unravel_index(g.reshape(-1).argmax(), g.shape)
    assert (int(k[0]), int(k[1]), int(k[2])) == (R.G_PLANT, 0, 0)               # the largest gradient is a SIGMA component
    assert float(inp["d_rgb"].abs().argmax() // 3) == R.G_PLANT


def test_largest_gradient_is_in_either_kind_of_component(table):
    """gmax_bits is max |d_sig_rgb| over all four components: the table must hold cases whose maximum is a sigma component and cases
    whose maximum is a colour component (a kernel that tracked only one kind would be right on the other cases by luck)."""
    comps = set()
    for name, (_, ref) in table.items():
        g = ref["d_sig_rgb"].abs()
        comps.add("sigma" if int(g.reshape(-1).argmax()) % 4 == 0 else "colour")
    assert comps == {"sigma", "colour"}


@pytest.mark.parametrize("name", list(R.CASES))
def test_fp32_oracle_within_half_of_every_tolerance(table, name):
    inp, ref = table[name]
    for k in R.OUTPUTS:
        assert bool(torch.isfinite(ref[k]).all()), (name, k)
    got = R.oracle32(inp)
    for k in R.OUTPUTS:
        assert bool(torch.isfinite(got[k]).all()), (name, k)
    errs, bad = R.compare(name + ", fp32 oracle at half the bars", got, ref, tol_scale=0.5)
    print(R.line(name + ", fp32 oracle", errs))
    assert not bad, "\n".join(bad)


def test_magnitudes_are_those_the_tolerances_assume(table):
    for name, (_, ref) in table.items():
        assert float(ref["rgb"].abs().max()) <= 1.0 + 1e-6 and float(ref["opacity"].max()) <= 1.0 + 1e-6 and float(ref["w_sel"].max()) <= 1.0 + 1e-6
        assert float(ref["depth"].max()) <= 8.2
        assert float(ref["d_sig_rgb"].abs().max()) <= 6.5, name


@pytest.mark.parametrize("white_back", [True, False])
@pytest.mark.parametrize("rows", [False, True])
def test_reference_gradient_by_central_differences(white_back, rows):
    N, S = 3, 5
    g = torch.Generator().manual_seed(7)
    sr = torch.cat([torch.randn(N, S, 1, generator=g, dtype=torch.float64) * 2.0, torch.rand(N, S, 3, generator=g, dtype=torch.float64)], -1)
    sr[1, -1, 0] = -23.0
    d = torch.randn(N, 3, generator=g)
    z = (1.0 + 7.0 * torch.rand(N, S, generator=g)).sort(dim=1).values if rows else torch.linspace(1, 8, S)
    if rows:
        z[2, 3] = z[2, 2]
    z32 = R.depths(z, torch.rand(N, generator=g) * 0.1, N)
    eps, eps_sel = torch.randn(N, S, generator=g), torch.randn(N, S, generator=g)
    d_rgb = torch.randn(N, 3, generator=g, dtype=torch.float64)
    f = lambda x: float((R.forward(x, d, z32, eps, eps_sel, white_back)["rgb"] * d_rgb).sum())
    leaf = sr.clone().requires_grad_(True)
    (R.forward(leaf, d, z32, eps, eps_sel, white_back)["rgb"] * d_rgb).sum().backward()
    h = 1e-6
    num = torch.zeros_like(sr)
    for i in range(sr.numel()):
        e = torch.zeros(sr.numel(), dtype=torch.float64)
        e[i] = h
        e = e.view_as(sr)
        num.view(-1)[i] = (f(sr + e) - f(sr - e)) / (2 * h)
    # central differences in fp64: truncation h^2 f''' / 6 ~ 1e-12, rounding 1e-16 / h ~ 1e-10
    assert float((num - leaf.grad).abs().max()) < 1e-8
    assert float(leaf.grad.abs().max()) > 1e-2
