"""tests/camera_ref.py checked without a GPU.

The bars of tests/test_camera_ops_gpu.py are c * 2^-24 * abs_sum with the constants of camera_ref.TOL.  They mean something only if
plain fp32 arithmetic meets them with room to spare: on EVERY case of the shared table, and on every setting of the upstream matrix,
the fp32 oracle with fp32 autograd must lie within HALF of each bar of the fp64 restatement, and each constant must be the smallest
power of two for which it does.  A case that breaks this gets other inputs, never another bar.  The restatement's gradient is checked
against central differences of its own forward, its closed-form Kinv against a numerical inverse, and abs_sum against the values it
bounds.  The bars are also held against those of test_a_ops_gpu.py::test_camera_parametrisation_fwd_bwd, which they replace at the
op level: on the cameras with theta <= 2 they must not be looser."""
import math

import pytest
import torch

import camera_ref as R

SETTINGS = [(name, "all") for name in R.CASES] + [(R.MATRIX_CASE, m) for m in R.MATRIX if m != "all"]


@pytest.fixture(scope="module")
def table():
    """case -> inputs, computed once and shared."""
    return {name: R.make(name) for name in R.CASES}


@pytest.fixture(scope="module")
def measured(table):
    """(case, matrix setting) -> (fp64 reference, compare() of the fp32 oracle at half the bars)."""
    out = {}
    for name, m in SETTINGS:
        ref = R.reference(table[name], R.MATRIX[m])
        out[name, m] = (ref, R.compare(f"{name}, {m}, fp32 oracle at half the bars", R.oracle32(table[name], R.MATRIX[m]), ref, tol_scale=0.5))
    return out


def test_case_table_covers_the_issue():
    c = R.CASES
    assert len(c) == 5 * 2 * 2 * 2
    assert {(v["C"], v["P"], v["H"], v["W"], v["neg"]) for v in c.values()} == {
        (C, P, H, W, n) for C in (1, 63, 64, 65, 130) for P in (1, 5) for H, W in ((600, 800), (800, 800)) for n in (False, True)}
    assert len({v["seed"] for v in c.values()}) == len(c)
    assert R.THETAS == (0.0, 1e-30, 1e-20, 3e-19, 1e-8, 1e-4, 1e-2, 0.5, 1.0, 2.0, 3.1, R.PI32, 4.5)
    assert R.PI32 == float(torch.tensor(math.pi, dtype=torch.float32)) != math.pi
    # both 64-camera blocks of the 130-camera cases see every regime, in both pose sets
    for th in R.thetas(130):
        assert set(th[:64]) == set(th[64:128]) == set(R.THETAS)
    assert all(a != b for a, b in zip(*R.thetas(130)))
    # the upstream matrix: each alone, all, none, on the 65-camera case
    assert c[R.MATRIX_CASE]["C"] == 65 and c[R.MATRIX_CASE]["P"] == 5
    assert {frozenset(v) for v in R.MATRIX.values()} == {frozenset((u,)) for u in R.UPSTREAMS} | {frozenset(R.UPSTREAMS), frozenset()}


def test_inputs_are_as_described(table):
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    assert float(f32(1e-30) * f32(1e-30)) == 0.0                                 # theta^2 underflows to 0 in fp32,
    assert 0.0 < float(f32(1e-20) * f32(1e-20)) < 2.0 ** -126                    # is denormal,
    assert 2.0 ** -126 < float(f32(3e-19) * f32(3e-19)) < 2.0 ** -123            # is just above the smallest normal number
    subnormal_squares = 0
    for name, inp in table.items():
        c = R.CASES[name]
        C, P = c["C"], c["P"]
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in inp.values() if isinstance(t, torch.Tensor)), name
        assert inp["wpose"].shape == inp["wpose_intr"].shape == (C, 6) and inp["wpts_intr"].shape == inp["wpts_extr"].shape == (C, P, 3)
        assert inp["dpix_intr"].shape == inp["dpix_extr"].shape == (C, P, 2) and (inp["H"], inp["W"]) == (c["H"], c["W"])
        th = R.thetas(C)
        for k, key in enumerate(("wpose", "wpose_intr")):
            got = inp[key][:, :3].double().norm(dim=-1)
            if th is None:
                assert 0.2 <= float(got.min()) and float(got.max()) <= 1.2 + 1e-6
            else:
                want = torch.tensor(th[k], dtype=torch.float64)
                assert bool(((got - want).abs() <= 1e-6 * want).all()), (name, key)
                sq = inp[key][:, :3] * inp[key][:, :3]
                subnormal_squares += int(((sq > 0) & (sq < 2.0 ** -126)).sum())
            assert float(inp[key][:, 3:].abs().max()) <= 1.0
        negs = R.neg_cameras(C)
        assert C < 4 or len(set(negs)) == 4
        for k, key in enumerate(("wfx", "wfy", "wux", "wuy")):
            w = inp[key]
            assert 0.7 - 1e-6 <= float(w.abs().min()) and float(w.abs().max()) <= 1.3 + 1e-6
            assert (w < 0).nonzero().reshape(-1).tolist() == ([negs[k]] if c["neg"] else []), (name, key)
        again = R.make(name)
        assert all(torch.equal(inp[k], again[k]) for k in inp if isinstance(inp[k], torch.Tensor))
    assert subnormal_squares > 0                           # theta = 1e-20 and 3e-19: squares w_i^2 that are denormal in fp32


def test_points_lie_in_front_of_both_poses(measured):
    for (name, m), (ref, _) in measured.items():
        if m == "all":
            for p2 in ref["p2"]:
                assert float(p2.min()) >= 0.5, (name, float(p2.min()))            # (placed 2 .. 6 in front; |p2| >= 0.5 is what is asked)


def test_closed_form_inverse_and_abs_sum(measured):
    for (name, m), (ref, _) in measured.items():
        if m == "all":
            inv = torch.linalg.inv(ref["K"])
            assert float((inv - ref["Kinv"]).abs().max()) <= 1e-12 * float(inv.abs().max()), name
        for k in R.OUTPUTS + R.GRADS:
            a = ref["abs_sum"][k]
            assert bool((a >= ref[k].abs() * (1 - 1e-12)).all()), (name, m, k)    # a sum of magnitudes bounds the sum
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(ref[k]).all())


@pytest.mark.parametrize("name,m", SETTINGS)
def test_fp32_oracle_within_half_of_every_bar(measured, name, m):
    _, (fracs, ratios, bad) = measured[name, m]
    print(R.line(f"{name}, {m}, fp32 oracle, half bars", fracs))
    assert not bad, "\n".join(bad)


def test_constants_are_the_smallest_powers_of_two(measured):
    worst = {}
    for (name, m), (_, (_, ratios, _)) in measured.items():
        for grp, r in ratios.items():
            if r > worst.get(grp, (0.0, ""))[0]:
                worst[grp] = (r, f"{name}, {m}")
    print("worst |fp32 oracle - fp64| / (2^-24 abs_sum):", {k: (round(v[0], 3), v[1]) for k, v in worst.items()})
    assert set(worst) == set(R.TOL)
    for grp, c in R.TOL.items():
        assert math.log2(c) == int(math.log2(c))
        assert c / 4 < worst[grp][0] <= c / 2, (grp, c, worst[grp])            # c holds at half the bar, c / 2 does not


def test_absent_upstream_leaves_exact_zeros(measured):
    for m, ups in R.MATRIX.items():
        ref, _ = measured[R.MATRIX_CASE, m]
        reached = {g for u in ups for g in R.REACHES[u]}
        for g in R.GRADS:
            if g in reached:
                assert float(ref[g].abs().min()) > 0.0, (m, g)
            else:
                assert int(torch.count_nonzero(ref[g])) == 0 and int(torch.count_nonzero(ref["abs_sum"][g])) == 0, (m, g)


def test_not_looser_than_the_bars_they_replace(table):
    """test_camera_parametrisation_fwd_bwd: 2e-6 on the poses, 2e-5 max(1, |g|_inf) on the gradients of ITS upstreams (dK, dKinv, dpose,
    dcalib; it has no reprojection branch).  On the cameras with theta <= 2 the new bars stay under them in every case."""
    ups = ("dK", "dKinv", "dpose", "dcalib")
    for name, inp in table.items():
        C = R.CASES[name]["C"]
        ref = R.reference(inp, ups)
        th = R.thetas(C)
        small = [torch.ones(C, dtype=torch.bool)] * 2 if th is None else [torch.tensor([t <= 2 for t in tt]) for tt in th]
        for key, sel in (("pose", small[0]), ("calib", small[1])):
            assert float(R.bar(key, ref)[sel].max()) <= 2e-6, (name, key)
        for key, sel in (("d_wpose", small[0]), ("d_wpose_intr", small[1])) + tuple((k, small[0] & small[1]) for k in R.GRADS[2:]):
            assert float(R.bar(key, ref)[sel].max()) <= 2e-5 * max(1.0, float(ref[key].abs().max())), (name, key)


def test_reference_gradient_by_central_differences(table):
    inp = table["C1_P5_600x800_neg"]                       # the negative multipliers sit in its one camera: sign(x) of |x| is in
    assert all(float(inp[k][0]) < 0 for k in ("wfx", "wfy", "wux", "wuy"))
    ref = R.reference(inp)

    def f(par):
        out = R.forward(par, inp["wpts_intr"], inp["wpts_extr"], inp["H"], inp["W"])
        return float(sum((out[o] * inp[u].double()).sum() for o, u in zip(R.OUTPUTS, R.UPSTREAMS)))
    base = {k: inp[k].double() for k in R.PARAMS}
    h = 1e-6
    for k in R.PARAMS:
        num = torch.zeros_like(base[k])
        for i in range(num.numel()):
            e = torch.zeros(num.numel(), dtype=torch.float64)
            e[i] = h
            e = e.view_as(num)
            num.view(-1)[i] = (f({**base, k: base[k] + e}) - f({**base, k: base[k] - e})) / (2 * h)
        g = ref["d_" + k]
        # central differences in fp64: truncation h^2 f''' / 6 ~ 1e-12 |g|, rounding 1e-16 |f| / h with |f| ~ |g|
        assert float((num - g).abs().max()) <= 1e-6 * float(g.abs().max()), (k, num, g)
        assert float(g.abs().max()) > 1e-2
