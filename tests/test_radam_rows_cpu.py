"""The row-lazy RAdam (`"lazy_rows": True` param groups) without a GPU: the param-group key; the semantics through the host
path `RAdam._step_host_rows` (independence of the rows, identity with the dense step when every row is visited, untouched rows); the
step-size table; the state-dict round trip; `MC_Model.optimizer_groups`; the entry point in the header, the ctypes table and the built
library, and its refusals ahead of any device work."""
import ctypes
import os
import re

import pytest
import torch

import radam_rows_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mcnerf_radam_rows_step"
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------------------------ the key
def test_lazy_rows_key_is_accepted_and_a_scalar_is_refused():
    from mc_nerf_amd.model import RAdam
    a, b = torch.nn.Parameter(torch.ones(5, 3)), torch.nn.Parameter(torch.ones(4))
    opt = RAdam([{"params": [a]}, {"params": [b], "lazy_rows": True}], lr=1e-3)
    assert [g["lazy_rows"] for g in opt.param_groups] == [False, True]
    assert RAdam([a, b]).param_groups[0]["lazy_rows"] is False                      # the default is the dense step
    a.grad, b.grad = torch.ones_like(a), torch.tensor([0.0, 1.0, 0.0, -0.0])
    opt.step()
    assert "row_step" not in opt.state[a] and opt.state[b]["row_step"].dtype == torch.int32
    assert opt.state[b]["row_step"].tolist() == [0, 1, 0, 0] and opt.state[b]["step"] == 1
    scalar = torch.nn.Parameter(torch.tensor(1.0))
    with pytest.raises(ValueError, match="lazy_rows"):
        RAdam([{"params": [a, scalar], "lazy_rows": True}])
    with pytest.raises(ValueError, match="lazy_rows"):
        opt.add_param_group({"params": scalar, "lazy_rows": True})
    RAdam([{"params": [scalar]}])                                                   # a dense group takes it, as today
    opt.add_param_group({"params": torch.nn.Parameter(torch.ones(2)), "lazy_rows": True})


# ------------------------------------------------------------------------------------------------------------------ the semantics
@pytest.fixture(scope="module")
def sparse_run():
    ps0, sched = X.params(), X.sparse_schedule()
    opt, ps, snaps = X.run(ps0, sched, CPU, lazy=True, each_step=True)
    return ps0, sched, opt, ps, snaps


def test_the_schedule_holds_the_cases_it_promises():
    sched = X.sparse_schedule()
    assert len(sched) == X.STEPS == 12 and not any(bool(X.visited(g).any()) for g in sched[X.ZERO_STEP])
    for ti, shape in enumerate(X.SHAPES):
        R = shape[0]
        visits = sum(X.visited(gs[ti]).int() for gs in sched)
        assert int(visits.max()) >= 6 and (R == 1 or int(visits.min()) < 6)          # some rows cross t = 6, others never do
        if R > 1:
            assert int(visits[R - 1]) == 0                                           # the row that is never visited
        g = X.rows_of(sched[2][ti])[1 % R]
        assert float(g[-1]) != 0.0 and int((g != 0).sum()) == 1                      # only its last element
        g = X.rows_of(sched[3][ti])[2 % R]
        assert bool(torch.signbit(g).all()) and not bool(X.visited(sched[3][ti])[2 % R])      # only -0.0: not a visit
        g = X.rows_of(sched[4][ti])[3 % R]
        assert int((g != 0).sum()) == 1 and 0 < float(g[0]) < 1.1754944e-38 and bool(X.visited(sched[4][ti])[3 % R])


def test_rows_are_independent_optimisers_on_the_host(sparse_run):
    """Equality is demanded: `_step_host_rows` runs `_step_host`'s torch ops on the gathered rows, and an element's result does not
    depend on where in a tensor it sits."""
    ps0, sched, _, _, snaps = sparse_run
    ref = X.per_row_dense(ps0, sched, CPU)
    for ti, (got, want) in enumerate(zip(snaps[-1], ref)):
        for a, b, what in zip(got, want, ("p", "exp_avg", "exp_avg_sq", "row_step")):
            assert torch.equal(a, b), (X.SHAPES[ti], what)


def test_all_rows_visited_is_the_dense_step_on_the_host():
    ps0, sched = X.params(), X.dense_schedule()
    _, _, lazy = X.run(ps0, sched, CPU, lazy=True)
    _, _, dense = X.run(ps0, sched, CPU, lazy=False)
    for ti, (a, b) in enumerate(zip(lazy, dense)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), X.SHAPES[ti]
        assert b[3] is None and torch.equal(a[3], torch.full((X.SHAPES[ti][0],), len(sched), dtype=torch.int32))


def test_unvisited_rows_keep_their_bits_on_the_host(sparse_run):
    ps0, sched, _, _, snaps = sparse_run
    for ti, p0 in enumerate(ps0):
        prev = (p0, torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros(p0.shape[0], dtype=torch.int32))
        for step, gs in enumerate(sched):
            vis = X.visited(gs[ti])
            now = snaps[step][ti]
            for a, b in zip(now, prev):
                assert X.same_bits(a[~vis], b[~vis]), (X.SHAPES[ti], step)
            assert torch.equal(now[3], prev[3] + vis.int())
            assert bool((X.rows_of(now[0])[vis] != X.rows_of(prev[0])[vis]).any(dim=1).all())      # and the visited ones moved
            prev = now


def test_weight_decay_acts_at_visits_only():
    from mc_nerf_amd.model import RAdam
    p = torch.nn.Parameter(torch.ones(3, 2))
    opt = RAdam([{"params": [p], "lazy_rows": True}], lr=1e-2, weight_decay=0.5)
    for _ in range(8):
        p.grad = torch.tensor([[1.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
        opt.step()
    assert torch.equal(p.detach()[1:], torch.ones(2, 2)) and float(p.detach()[0, 1]) < 1.0 and opt.state[p]["row_step"].tolist() == [8, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.0, 0.99)])
@pytest.mark.parametrize("degenerate", [True, False])
def test_table_is_the_rectification_of_every_step(betas, degenerate, monkeypatch):
    from mc_nerf_amd.model import RAdam
    monkeypatch.setattr(RAdam, "ROW_TABLE_CAPACITY", 4)
    p = torch.nn.Parameter(torch.ones(2, 2))
    opt = RAdam([{"params": [p], "lazy_rows": True}], betas=betas, degenerated_to_sgd=degenerate)
    ent = opt._row_table(0, opt.param_groups[0], CPU, 50)
    assert ent["T"] == 64 and ent["table"].shape == (64, 2) and ent["table"].dtype == torch.float32
    for t in range(1, 51):
        n_sma, ss = RAdam._rectification(t, betas[0], betas[1], degenerate)
        want = torch.tensor([1.0 if n_sma >= 5 else 0.0, ss], dtype=torch.float32)
        assert torch.equal(ent["table"][t - 1], want), t
    assert opt._row_table(0, opt.param_groups[0], CPU, 64) is ent                      # no copy while it is large enough
    assert opt._row_table(0, opt.param_groups[0], CPU, 65)["T"] == 128                 # grown by doubling
    opt.param_groups[0]["betas"] = (0.5, 0.9)                                          # other betas: rebuilt
    ent2 = opt._row_table(0, opt.param_groups[0], CPU, 3)
    assert ent2["key"][:2] == (0.5, 0.9) and float(ent2["table"][2, 1]) == pytest.approx(RAdam._rectification(3, 0.5, 0.9, degenerate)[1], rel=1e-6)
    opt.degenerated_to_sgd = not degenerate
    assert opt._row_table(0, opt.param_groups[0], CPU, 3) is not ent2


# ------------------------------------------------------------------------------------------------------------------ the state dict
def test_state_dict_round_trip_on_the_host():
    from mc_nerf_amd.model import RAdam
    ps0, sched = X.params(), X.sparse_schedule(steps=9)
    _, _, whole = X.run(ps0, sched, CPU, lazy=True)
    opt, ps, _ = X.run(ps0, sched[:5], CPU, lazy=True)
    sd = opt.state_dict()
    assert all(s["row_step"].dtype == torch.int32 for s in sd["state"].values())
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = RAdam([{"params": ps2, "lazy_rows": True}], **X.HYPER)
    opt2.load_state_dict(sd)
    for p, q in zip(ps, ps2):
        rs = opt2.state[q]["row_step"]
        assert rs.dtype == torch.int32 and torch.equal(rs, opt.state[p]["row_step"]) and rs.data_ptr() != opt.state[p]["row_step"].data_ptr()
    assert opt2.param_groups[0]["lazy_rows"] is True
    for gs in sched[5:]:
        for q, g in zip(ps2, gs):
            q.grad = g
        opt2.step()
    for a, b in zip(X.snapshot(opt2, ps2), whole):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("kw, n_keys", [({}, 46), ({"color_calib": "affine"}, 47), ({"color_calib": "affine", "lens_model": "radial"}, 48)])
def test_optimizer_groups_partition_the_parameters_exactly_once(kw, n_keys):
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd.model import MC_Model, RAdam
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    sp.update(kw)
    model = MC_Model(sp)
    named = list(model.named_parameters())
    assert len(named) == n_keys == len(model.state_dict())
    nerf, cams = model.optimizer_groups()
    assert set(nerf) == {"params"} and set(cams) == {"params", "lazy_rows"} and cams["lazy_rows"] is True
    assert model.optimizer_groups(lazy_cameras=False)[1]["lazy_rows"] is False
    assert [id(p) for p in nerf["params"]] == [id(p) for n, p in named if n.startswith("nerf.")]
    assert [id(p) for p in cams["params"]] == [id(p) for n, p in named if not n.startswith("nerf.")]
    assert len(nerf["params"]) == 40 and len(cams["params"]) == n_keys - 40
    assert sorted(id(p) for p in nerf["params"] + cams["params"]) == sorted(id(p) for _, p in named)
    assert all(p.shape[0] == model.train_numb for p in cams["params"])
    opt = RAdam(model.optimizer_groups(), lr=1e-3)
    assert [g["lazy_rows"] for g in opt.param_groups] == [False, True]
    assert RAdam(model.parameters()).param_groups[0]["lazy_rows"] is False


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_declares_the_entry_point_and_keeps_its_version():
    from mc_nerf_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "mcnerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "optim_rows.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "optim_rows.hip"))
    assert "mcnerf_optim_rows.h" in build.HEADERS and os.path.isfile(os.path.join(build.CSRC, "mcnerf_optim_rows.h"))
    lib = ctypes.CDLL(build.build(verbose=False))
    assert f"int {NAME}(" in code and hasattr(lib, NAME)
    n_args = code.split(f"int {NAME}(")[1].split(")")[0].count(",") + 1
    assert len(_lib.SIGNATURES[NAME][1]) == n_args == 18
    assert _lib.ABI_VERSION == 7                             # (new symbols only; tests/test_abi_cpu.py checks header, table and library)


def test_digested_kernel_sources_do_not_include_the_new_files():
    import bench
    from mc_nerf_amd import build
    assert not {"optim_rows.hip", "mcnerf_optim_rows.h"} & set(bench.MLP_KERNEL_SOURCES)
    for f in bench.MLP_KERNEL_SOURCES:
        text = open(os.path.join(build.CSRC, f)).read()
        assert "optim_rows" not in text and "radam_rows" not in text, f


# ------------------------------------------------------------------------------------------------------------------ refusals
PTRS = ["params", "grads", "exp_avg", "exp_avg_sq", "row_step", "n_rows", "row_len", "table"]


def _call(l, *, n=2, missing=(), null_entry=None, n_rows=(3, 5), row_len=(6, 1), T=8):
    """The device pointers are never read: a host buffer stands in for them."""
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    k = max(n, 1)
    arr = lambda name: None if name in missing else ctypes.cast((ctypes.c_void_p * k)(*[None if (name, i) == null_entry else p for i in range(k)]), ctypes.c_void_p)
    sizes = lambda name, v: None if name in missing else ctypes.cast((ctypes.c_longlong * len(v))(*v), ctypes.c_void_p)
    return l.mcnerf_radam_rows_step(n, arr("params"), arr("grads"), arr("exp_avg"), arr("exp_avg_sq"), arr("row_step"),
                                    sizes("n_rows", n_rows), sizes("row_len", row_len), 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                    None if "table" in missing else p, T, p, 1, None)


def _refused(l, rc):
    return rc != 0 and f"{NAME}: invalid argument".encode() in l.mcnerf_last_error()


@pytest.mark.parametrize("missing", PTRS)
def test_entry_point_refuses_null_pointers_without_a_gpu(missing):
    """The refusals sit ahead of any HIP call: non-zero on a machine without a GPU."""
    from mc_nerf_amd import _lib
    l = _lib.lib()
    assert _refused(l, _call(l, missing=(missing,))), missing


@pytest.mark.parametrize("name", PTRS[:5])
def test_entry_point_refuses_a_null_table_entry_without_a_gpu(name):
    from mc_nerf_amd import _lib
    l = _lib.lib()
    assert _refused(l, _call(l, null_entry=(name, 1))), name


def test_entry_point_refuses_bad_scalars_without_a_gpu():
    from mc_nerf_amd import _lib
    l = _lib.lib()
    assert _refused(l, _call(l, n=-1))
    assert _refused(l, _call(l, n_rows=(3, 0))) and _refused(l, _call(l, n_rows=(-1, 5)))
    assert _refused(l, _call(l, row_len=(0, 1))) and _refused(l, _call(l, row_len=(6, -2)))
    assert _refused(l, _call(l, T=0)) and _refused(l, _call(l, T=-4))
    assert _call(l, n=0) == 0                                                         # nothing to do is not an error, and launches nothing
