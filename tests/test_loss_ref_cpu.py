"""tests/loss_ref.py checked without a GPU.

The bars of tests/test_loss_ops_gpu.py (loss_ref.TOL: 2e-6 max(1, |value|), 2e-6 max |gradient| + 1e-12, against fp64) are
meaningful only if plain fp32 arithmetic meets them with room to spare: on EVERY case of the shared table fp32 eager torch must lie
within HALF of each bar of the fp64 restatement.  A case that breaks this gets other inputs, never another bar.  The restatement's
gradients are also checked against their closed forms, so that they rest on more than autograd of itself."""
import pytest
import torch

import loss_ref as R


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
    assert (R.H, R.W) == (600, 800)
    assert [c[f"rays_{n}"]["n"] for n in R.N_RAYS] == [1, 85, 86, 341, 342, 7001, 43690, 43691, 70001]
    assert [c[f"points_{p}"]["np"] for p in R.N_POINTS] == [0, 1, 255, 256, 257, 550] and all(c[f"points_{p}"]["n"] == 342 for p in R.N_POINTS)
    flags = {(v["n"], v["normalise"], v["with_fine"]) for k, v in c.items() if k.startswith("flags_")}
    assert flags == {(n, a, b) for n in (86, 7001, 43691) for a in (True, False) for b in (True, False)}
    cells = [v for k, v in c.items() if k.startswith("flags_")]
    assert len({v["seed"] for v in cells}) == len(cells) == 12 and all(v["np"] == 550 for v in cells)
    # the launch geometry the ray counts sit on
    assert 3 * 85 == 255 and 3 * 86 == 258 and R.LOSS_THREADS == 256
    assert [R.blocks_of(n) for n in (1, 341, 342, 7001, 43690, 43691, 70001)] == [1, 1, 2, 21, 128, 128, 128]
    assert 3 * 43690 == 128 * 1024 - 2 and 3 * 43691 == 128 * 1024 + 1             # the last size without and the first with a second round
    assert R.REPROJ_N == (1, 255, 256, 257, 550, 1000) and R.DLOSS == 0.37 and R.SCALE3_G == 0.37
    assert R.SCALE3_CASES == ((None, 5, None), (300, 5, 0), (5, 300, 257), (256, 256, 256), (1100, 21003, 21003))


def test_inputs_are_as_described(table):
    for name, (inp, _) in table.items():
        c = R.CASES[name]
        assert inp["rgb_c"].shape == inp["gt"].shape == (c["n"], 3) and (inp["rgb_f"] is not None) == c["with_fine"]
        assert (inp["pd"] is None) == (inp["pt_gt"] is None) == (c["np"] == 0)
        if c["np"]:
            assert inp["pd"].shape == inp["pt_gt"].shape == (c["np"], 2)
            assert float(inp["pt_gt"][:, 0].max()) <= R.W and float(inp["pt_gt"][:, 1].max()) <= R.H and float(inp["pt_gt"].min()) >= 0
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in inp.values() if isinstance(t, torch.Tensor))
        again = R.make(name)
        assert all(torch.equal(inp[k], again[k]) for k in inp if isinstance(inp[k], torch.Tensor))


@pytest.mark.parametrize("name", list(R.CASES))
def test_fp32_eager_within_half_of_every_bar(table, name):
    inp, ref = table[name]
    fracs, bad = R.compare(name + ", fp32 eager at half the bars", R.eager32(inp), ref, tol_scale=0.5)
    print(R.line(name + ", fp32 eager, half bars", fracs))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", R.REPROJ_N)
def test_fp32_eager_reprojection_loss_within_half_of_every_bar(n):
    inp = R.make_reproj(n)
    fracs, bad = R.compare(f"reproj_loss n = {n}, fp32 eager at half the bars", R.reproj_eager32(inp), R.reproj_reference(inp), tol_scale=0.5,
                           values=("value",), grads=("d_pd",))
    print(R.line(f"reproj_loss n = {n}, fp32 eager, half bars", fracs))
    assert not bad, "\n".join(bad)


def test_reference_against_the_closed_forms(table):
    for name, (inp, ref) in table.items():
        c = R.CASES[name]
        gt = inp["gt"].double()
        assert float((ref["d_c"] - 2.0 * (inp["rgb_c"].double() - gt) / (3 * c["n"])).abs().max()) <= 1e-15
        assert (ref["d_f"] is None) == (not c["with_fine"])
        if c["with_fine"]:
            assert float((ref["d_f"] - 2.0 * (inp["rgb_f"].double() - gt) / (3 * c["n"])).abs().max()) <= 1e-15
        if c["np"] == 0:
            assert ref["d_pd"] is None and float(ref["l_intr"]) == 0.0 and float(ref["total"]) == float(ref["rgb"])
            continue
        e = inp["pd"].double() - inp["pt_gt"].double()
        li = float((e[:, 0] ** 2).mean() / R.W ** 2 + (e[:, 1] ** 2).mean() / R.H ** 2)
        s = 1.0 / (li + 1e-8) if c["normalise"] else 1.0                     # the denominator is a constant: d total / d L_intr
        want = s * 2.0 * e / c["np"] / torch.tensor([float(R.W) ** 2, float(R.H) ** 2], dtype=torch.float64)
        assert float((ref["d_pd"] - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert abs(float(ref["l_intr"]) - li) <= 1e-15 and abs(float(ref["total"]) - (li * s + float(ref["rgb"]))) <= 1e-14
        if c["normalise"]:
            assert 0.99 < float(ref["total"]) - float(ref["rgb"]) < 1.0     # L_intr / (L_intr + 1e-8): just under 1
