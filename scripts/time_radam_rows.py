"""Times the row-lazy RAdam of the per-camera parameters (`"lazy_rows": True` param groups).

    python scripts/time_radam_rows.py [out.txt] [--rays N] [--img S] [--steps N] [--windows N]        (needs the GPU)

Two measurements, both with device events and nothing but the measured work between them:
  * the update launch alone on the eight camera tensors of a model with colour calibration and a lens (C = 110: [C,6] x 3, [C] x 4,
    [C,2]): mcnerf_radam_rows_step with one camera's rows visited and with every row visited, next to the dense mcnerf_radam_step
    (phase 4: the update alone) on the same tensors, ctypes arguments built once, alternating inside every round; and the whole
    RAdam.step() (clear + check + update) of a dense and of a lazy group on these tensors;
  * the full train step (forward, loss, backward, RAdam) at the bench shape (Ball rig, 110 cameras, 32768 rays, 64 x 2 samples,
    f16x3h, random-init selection): RAdam(model.parameters()) -- the step of the commit before this feature --, and
    RAdam(model.optimizer_groups(lazy_cameras=False / True)), alternating windows, one model each from one seed.
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mc_nerf_amd import _lib, synthetic as S  # noqa: E402
from mc_nerf_amd.data import DeviceImageSet  # noqa: E402
from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, RAdam  # noqa: E402


def opt_arg(name, default, cast):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    if not torch.cuda.is_available():
        sys.exit("time_radam_rows.py measures on the GPU; there is none here")
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    rays, img = opt_arg("--rays", 32768, int), opt_arg("--img", 800, int)
    steps, windows, warm = opt_arg("--steps", 20, int), opt_arg("--windows", 3, int), opt_arg("--warmup", 8, int)
    dev = torch.device("cuda:0")
    H = W = img
    C = 110
    g = torch.Generator().manual_seed(0)
    shapes = [(C, 6), (C, 6), (C,), (C,), (C,), (C,), (C, 6), (C, 2)]
    hyper = dict(lr=1e-3, weight_decay=4e-4)

    def camera_optimiser(lazy):
        ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]
        opt = RAdam([{"params": ps, "lazy_rows": lazy}], **hyper)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).to(dev)
        opt.step()                          # the state, the guard and the table exist from here on
        return opt, ps

    def set_grads(ps, one_camera):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).to(dev)
            if one_camera:
                p.grad[:7] = 0.0
                p.grad[8:] = 0.0

    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    fns = {}
    keep = []
    for name, lazy, one in (("radam_step (dense update)", False, True), ("radam_rows_step, 1 of 110 rows", True, True),
                            ("radam_rows_step, all rows", True, False)):
        opt, ps = camera_optimiser(lazy)
        set_grads(ps, one)
        group = opt.param_groups[0]
        (p_arr, g_arr, m_arr, v_arr, sizes), grads = opt._bucket_tables(ps)
        cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
        guard = opt._guard[dev].data_ptr()
        b1, b2 = group["betas"]
        common = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
        if lazy:
            n = len(ps)
            rs = (ctypes.c_void_p * n)(*[opt.state[p]["row_step"].data_ptr() for p in ps])
            nr = (ctypes.c_longlong * n)(*[p.shape[0] for p in ps])
            rl = (ctypes.c_longlong * n)(*[p.numel() // p.shape[0] for p in ps])
            ent = opt._row_table(0, group, dev, 1)
            args = (n, cast(p_arr), cast(g_arr), cast(m_arr), cast(v_arr), cast(rs), cast(nr), cast(rl), *common, ent["table"].data_ptr(),
                    int(ent["T"]), guard, 0, stream)
            fn = lib.mcnerf_radam_rows_step
            keep.append((rs, nr, rl, ent))
        else:
            n_sma, ss = RAdam._rectification(2, b1, b2, True)
            args = (len(ps), cast(p_arr), cast(g_arr), cast(m_arr), cast(v_arr), cast(sizes), *common, float(ss), int(n_sma >= 5), guard, 4, stream)
            fn = lib.mcnerf_radam_step
        keep.append((opt, ps, grads, p_arr, g_arr, m_arr, v_arr, sizes))
        fns[name] = (lambda fn, args: lambda i: fn(*args))(fn, args)
    for name, lazy in (("RAdam.step(), dense group", False), ("RAdam.step(), lazy group", True)):
        opt, ps = camera_optimiser(lazy)
        set_grads(ps, True)
        fns[name] = (lambda opt: lambda i: opt.step())(opt)
        keep.append((opt, ps))
    for f in fns.values():
        timed(f, 50)
    us = {k: [] for k in fns}
    for w in range(windows):
        for k, f in fns.items():
            us[k].append(1e3 * timed(f, 200))
    lines = [f"row-lazy RAdam of the per-camera parameters, one MI355X: the eight camera tensors at C = {C} ([C,6] x 3, [C] x 4, [C,2]; {sum(torch.Size(s).numel() for s in shapes)} floats);",
             f"one launch per call on ctypes arguments built once (RAdam.step(): clear + check + update through Python), 200 back-to-back calls per window (device events), {windows} windows, alternating"]
    for k, v in us.items():
        lines.append(f"{k:32s}: " + "  ".join(f"{x:7.2f}" for x in v) + f"  us per call   (min {min(v):.2f})")

    configs = {"parameters()": None, "groups, dense": False, "groups, lazy": True}
    images = DeviceImageSet.synthetic(C, H, W, dev, channels=4, seed=7)
    runs = {}
    wpts = pts = None
    for name, lazy in configs.items():
        torch.manual_seed(42)
        sp = S.make_sys_param(dev, samples=64, scale=2, batch=rays, H=H, W=W, barf_mask=False, precision="f16x3h")
        model = MC_Model(sp).to(dev)
        S.init_cameras_near_gt(model, noise=1e-3)
        if runs:                            # one workspace pool for all models: their steps never overlap, the keys are the same
            model.nerf.ws_pool = next(iter(runs.values()))["model"].nerf.ws_pool
        model.nerf.reserve_workspaces(rays)
        if wpts is None:
            wpts, pts = (v.to(dev) for v in S.calibration_points(sp["gt_pose"], sp["intr_mat"][0]))
        params = model.parameters() if lazy is None else model.optimizer_groups(lazy_cameras=lazy)
        runs[name] = dict(model=model, loss=MC_NeRF_Loss(sp), opt=RAdam(params, lr=5e-4, weight_decay=4e-4))
    order = torch.randperm(C * 64, generator=torch.Generator().manual_seed(1)) % C      # the camera ids of the steps, host side

    def step_of(name):
        q = runs[name]

        def step(i):
            cams = order[i % (order.numel() - 1):][:1]
            loss_dict, *_ = q["model"]((images, cams, wpts, pts, wpts, pts), 20, "GLOBAL_OPTIM_EPOCH", 0.6)
            loss = q["loss"](loss_dict, "GLOBAL_OPTIM_EPOCH")
            q["opt"].zero_grad(set_to_none=True)
            loss.backward()
            q["opt"].step()
        return step

    steps_of = {name: step_of(name) for name in runs}
    for name in runs:
        timed(steps_of[name], warm)
    ms = {name: [] for name in runs}
    for w in range(windows):
        for name in runs:
            ms[name].append(timed(lambda i: steps_of[name](warm + w * steps + i), steps))
    lines.append(f"full train step, Ball rig {H}x{W}, {rays} rays, 64x2 samples, f16x3h, random-init selection, one camera per step; {windows} windows of {steps} steps each,")
    lines.append("alternating; RAdam(model.parameters()) is the step before this feature, 'groups' = RAdam(model.optimizer_groups(lazy_cameras=...)):")
    for name, v in ms.items():
        lines.append(f"step  {name:16s}: " + "  ".join(f"{x:7.3f}" for x in v) + f"  ms/step   (min {min(v):.3f}, max {max(v):.3f})")
    off = "parameters()"
    for on in ("groups, dense", "groups, lazy"):
        lo, hi, m = min(ms[off]), max(ms[off]), sum(ms[on]) / len(ms[on])
        where = "inside" if lo <= m <= hi else f"{m - hi:.3f} ms above" if m > hi else f"{lo - m:.3f} ms below"
        lines.append(f"  '{on}' mean {m:.3f} ms: {where} the window spread of '{off}' [{lo:.3f}, {hi:.3f}]")
    skipped = {name: q["opt"].skipped_steps() for name, q in runs.items()}
    lines.append(f"refused steps: {skipped}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
