"""The row-lazy RAdam (`"lazy_rows": True` param groups; csrc/optim_rows.hip) on the GPU.

Shapes, schedules and runners are tests/radam_rows_cases.py's (its docstring lists the cases).  The equalities are torch.equal: the
kernel's element arithmetic is mcn_radam_element (csrc/mcnerf_optim_rows.h), the function radam_kernel calls, a wave owns its row, and nothing is atomic.  Against the host
path the gate is the 1e-6 of test_a_ops_gpu.py::test_fused_radam_matches_host_arithmetic (the host forms step_size * lr in double)."""
import pytest
import torch

import radam_rows_cases as X
from mc_nerf_amd import synthetic as S

pytestmark = pytest.mark.gpu
NAMES = ("p", "exp_avg", "exp_avg_sq", "row_step")


@pytest.fixture(scope="module")
def sparse_run(gpu_device):
    """The lazy run of the sparse schedule, computed once and left unchanged: (initial tensors, schedule, snapshots after every step)."""
    ps0, sched = X.params(), X.sparse_schedule()
    opt, _, snaps = X.run(ps0, sched, gpu_device, lazy=True, each_step=True)
    assert opt.skipped_steps() == 0
    return ps0, sched, snaps


# ------------------------------------------------------------------------------------------------------------------ 1
def test_all_rows_visited_is_the_dense_kernel_bit_for_bit(gpu_device):
    ps0, sched = X.params(), X.dense_schedule(steps=9)
    _, _, lazy = X.run(ps0, sched, gpu_device, lazy=True)
    _, _, dense = X.run(ps0, sched, gpu_device, lazy=False)
    for shape, a, b in zip(X.SHAPES, lazy, dense):
        for x, y, what in zip(a[:3], b[:3], NAMES):
            assert torch.equal(x, y), (shape, what)
        assert b[3] is None and a[3].dtype == torch.int32 and torch.equal(a[3].cpu(), torch.full((shape[0],), 9, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------ 2
def test_rows_are_independent_dense_optimisers(sparse_run, gpu_device):
    ps0, sched, snaps = sparse_run
    ref = X.per_row_dense(ps0, sched, gpu_device)
    for shape, got, want in zip(X.SHAPES, snaps[-1], ref):
        for a, b, what in zip(got, want, NAMES):
            assert torch.equal(a, b), (shape, what)


# ------------------------------------------------------------------------------------------------------------------ 3
def test_kernel_matches_the_host_path(sparse_run):
    ps0, sched, snaps = sparse_run
    _, _, host = X.run(ps0, sched, torch.device("cpu"), lazy=True)
    for shape, got, want in zip(X.SHAPES, snaps[-1], host):
        for a, b, what in zip(got[:3], want[:3], NAMES):
            err = float((a.cpu() - b).abs().max())
            print(f"[radam rows, {shape}] {what}: max |kernel - host| {err:.3e}")
            assert err < 1e-6, (shape, what)
        assert torch.equal(got[3].cpu(), want[3]), shape


# ------------------------------------------------------------------------------------------------------------------ 4
def test_unvisited_rows_keep_their_bits(sparse_run, gpu_device):
    ps0, sched, snaps = sparse_run
    for ti, p0 in enumerate(ps0):
        p0 = p0.to(gpu_device)
        prev = (p0, torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros(p0.shape[0], dtype=torch.int32, device=gpu_device))
        for step, gs in enumerate(sched):
            vis = X.visited(gs[ti]).to(gpu_device)
            now = snaps[step][ti]
            for a, b, what in zip(now, prev, NAMES):
                assert X.same_bits(a[~vis], b[~vis]), (X.SHAPES[ti], step, what)
            assert torch.equal(now[3], prev[3] + vis.int()), (X.SHAPES[ti], step)
            if step == X.ZERO_STEP:                                                    # nothing visited: everything unchanged
                assert not bool(vis.any()) and all(X.same_bits(a, b) for a, b in zip(now, prev))
            prev = now
        assert int(prev[3].max()) >= 6 and (p0.shape[0] == 1 or int(prev[3].min()) == 0)


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("lazy_first", [False, True])
def test_guard_refuses_the_whole_step_across_dense_and_lazy_groups(gpu_device, lazy_first):
    from mc_nerf_amd.model import RAdam
    dev = gpu_device
    gen = torch.Generator().manual_seed(4)
    dense = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in ((300, 7), (3,))]
    lazy = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in ((110, 6), (3, 130))]
    groups = [{"params": dense}, {"params": lazy, "lazy_rows": True}]
    opt = RAdam(groups[::-1] if lazy_first else groups, lr=1e-2, weight_decay=1e-3)
    every = dense + lazy

    def grads():
        for p in every:
            p.grad = torch.randn(p.shape, generator=gen).to(dev)
        lazy[0].grad[5:] = 0.0

    grads()
    opt.step()
    assert opt.skipped_steps() == 0 and opt.state[lazy[0]]["row_step"].tolist() == [1] * 5 + [0] * 105
    for k, (victim, where) in enumerate(((lazy[1], (2, 129)), (dense[0], (299, 6)))):
        before = X.snapshot(opt, every)
        grads()
        victim.grad[where] = float("nan")
        opt.step()                                                                     # refused, everywhere
        for p, a, b in zip(every, X.snapshot(opt, every), before):
            assert all(y is None or X.same_bits(x, y) for x, y in zip(a, b)), tuple(p.shape)
        assert opt.skipped_steps() == k + 1
    before = X.snapshot(opt, every)
    grads()
    opt.step()                                                                         # finite again: the update goes through
    assert opt.skipped_steps() == 2
    assert all(not torch.equal(a[0], b[0]) for a, b in zip(X.snapshot(opt, every), before))
    assert opt.state[lazy[0]]["row_step"].tolist() == [2] * 5 + [0] * 105 and opt.state[lazy[1]]["row_step"].tolist() == [2, 2, 2]
    assert all(bool(torch.isfinite(p).all()) for p in every)


# ------------------------------------------------------------------------------------------------------------------ 6
def test_table_growth_changes_nothing(gpu_device, monkeypatch):
    from mc_nerf_amd.model import RAdam
    ps0, sched = X.params(), X.sparse_schedule(steps=9)
    opt_a, _, a = X.run(ps0, sched, gpu_device, lazy=True)
    assert RAdam.ROW_TABLE_CAPACITY == 1024 and [e["T"] for e in opt_a._row_tables.values()] == [1024]
    monkeypatch.setattr(RAdam, "ROW_TABLE_CAPACITY", 4)
    opt_b, _, b = X.run(ps0, sched, gpu_device, lazy=True)
    assert [e["T"] for e in opt_b._row_tables.values()] == [16]                        # grown twice: at steps 5 and 9
    for shape, x, y in zip(X.SHAPES, a, b):
        assert all(torch.equal(u, v) for u, v in zip(x, y)), shape


# ------------------------------------------------------------------------------------------------------------------ 7
def test_state_dict_round_trip(gpu_device):
    from mc_nerf_amd.model import RAdam
    ps0, sched = X.params(), X.sparse_schedule(steps=9)
    _, _, whole = X.run(ps0, sched, gpu_device, lazy=True)
    opt, ps, _ = X.run(ps0, sched[:5], gpu_device, lazy=True)
    sd = opt.state_dict()
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = RAdam([{"params": ps2, "lazy_rows": True}], **X.HYPER)
    opt2.load_state_dict(sd)
    for p, q in zip(ps, ps2):
        rs = opt2.state[q]["row_step"]
        assert rs.dtype == torch.int32 and rs.device == q.device and q.is_cuda and torch.equal(rs, opt.state[p]["row_step"])
    for gs in sched[5:]:
        for q, g in zip(ps2, gs):
            q.grad = g.to(gpu_device)
        opt2.step()
    for shape, x, y in zip(X.SHAPES, X.snapshot(opt2, ps2), whole):
        assert all(torch.equal(u, v) for u, v in zip(x, y)), shape


# ------------------------------------------------------------------------------------------------------------------ 8. the model
STAGE = "GLOBAL_OPTIM_EPOCH"
H, W = 12, 20
BATCH = 301
STEP_CAMS = ([2, 0, 2], [5, 1, 5])               # the cameras of step 1 and of step 2


def _two_steps(dev, K, lazy):
    """A small MC_Model as tests/test_color_calib_gpu.py builds it, color_calib = "affine", two joint-stage steps on different cameras
    -> (model, optimiser, per step: the gradients and the values after the step of weights_pose / weights_color)."""
    from mc_nerf_amd.data import DeviceImageSet
    from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, RAdam
    extra = {"cams_per_step": K} if K > 1 else {}
    sp = S.make_sys_param(dev, samples=32, scale=2, batch=BATCH, H=H, W=W, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision="f16x3",
                          color_calib="affine", **extra)
    torch.manual_seed(3)
    model = MC_Model(sp).to(dev)
    # (se(3) noise 0.01: with the cameras exactly at the ground truth the fp32 reprojection residual of some cameras -- 2 of the 110 here --
    # is exactly zero, their rows of weights_pose_intr.grad with it, and the rule rightly does not visit them)
    S.init_cameras_near_gt(model, noise=0.01)
    with torch.no_grad():
        model.weights_color.copy_(0.6 * torch.rand(model.train_numb, 6, generator=torch.Generator().manual_seed(8)) - 0.3)
    u8 = torch.randint(0, 256, (model.train_numb, H * W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    images = DeviceImageSet(u8.to(dev), H, W)
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    loss_fn = MC_NeRF_Loss(sp)
    opt = RAdam(model.optimizer_groups(lazy_cameras=lazy), lr=5e-4, weight_decay=0.0)
    torch.manual_seed(7)
    steps = []
    for k, cams in enumerate(STEP_CAMS):
        data = (images, torch.tensor(cams[:K]), wpts, pts, wpts, pts)
        loss_dict, *_ = model(data, 20 + k, STAGE, 0.5)
        loss = loss_fn(loss_dict, STAGE)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        grads = {n: getattr(model, n).grad.detach().clone() for n in ("weights_pose", "weights_color")}
        opt.step()
        steps.append((grads, {n: getattr(model, n).detach().clone() for n in ("weights_pose", "weights_color")}))
    assert opt.skipped_steps() == 0
    return model, opt, steps


@pytest.mark.parametrize("K", [1, 3])
def test_model_steps_leave_the_other_cameras_rows_alone(gpu_device, K):
    model, opt, steps = _two_steps(gpu_device, K, lazy=True)
    C = model.train_numb
    assert [g["lazy_rows"] for g in opt.param_groups] == [False, True]
    for (grads, _), cams in zip(steps, STEP_CAMS):
        inside = sorted(set(cams[:K]))
        outside = [c for c in range(C) if c not in inside]
        for name, g in grads.items():            # the precondition: the rows of the cameras outside the step are exactly zero
            assert float(g[outside].abs().max()) == 0.0 and bool((g[inside] != 0).any(dim=1).all()), name
    first = sorted(set(STEP_CAMS[0][:K]))
    assert not set(first) & set(STEP_CAMS[1][:K])
    _, _, dense = _two_steps(gpu_device, K, lazy=False)
    for name in ("weights_pose", "weights_color"):
        assert X.same_bits(steps[1][1][name][first], steps[0][1][name][first]), name                  # post-step-1 bits
        assert bool((dense[1][1][name][first] != dense[0][1][name][first]).any(dim=1).all()), name     # the dense twin moved them
    rs = {n: opt.state[getattr(model, n)]["row_step"] for n in ("weights_pose", "weights_color", "weights_pose_intr")}
    assert all(r.dtype == torch.int32 and r.shape == (C,) for r in rs.values())
    assert torch.equal(rs["weights_pose_intr"].cpu(), torch.full((C,), 2, dtype=torch.int32))       # the dense reprojection term
    want = torch.zeros(C, dtype=torch.int32)
    want[sorted(set(STEP_CAMS[0][:K]) | set(STEP_CAMS[1][:K]))] = 1
    assert torch.equal(rs["weights_pose"].cpu(), want) and torch.equal(rs["weights_color"].cpu(), want)
