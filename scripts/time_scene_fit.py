#!/usr/bin/env python3
"""Cost of fitting the scene box to the voxel sigma cache (`ray_bounds_fit = "voxel"`).

    python scripts/time_scene_fit.py [--steps K] [--warmup W] [--rays R] [--out FILE]

One MI355X, one process.  Timed in this order:
  1. ops.voxel_box on its own at G = 128, 256 and 384 (20 calls between two HIP events; a call is three launches: the cells' identities,
     the pass over the grid, the finish), on a grid without an occupied cell, with 1 % and with every cell occupied: us per call and
     grid bytes / time, beside the 6.2 TB/s that dw16_stream_kernel reads at (profiles/r06_kernel_table_f16x3h.txt); the same call at
     G = 2 is the floor of the three launches, and a call within 3 us of it is printed as "at the floor", without a rate;
  2. ops.ray_depths with the box on the device beside the tuple form, R = 32768 rays, 64 + 128 depths, with and without the flag;
  3. the bench-shaped step (the nets of bench.py's default line, f16x3h, R rays of cameras at radius 4; render_rays_train, an MSE loss
     on both colours and the backward), voxel mode on a fresh grid with voxel_beta = 1e-6 (every cell stays occupied: the fitted box is
     the outer box, the cube, so both modes evaluate the same samples), `ray_bounds_fit` "fixed" against "voxel" in three alternating
     windows.  The spread of the windows of one mode is the margin a difference must exceed to be called one; the fit mode's windows hold
     one or two fits each (every 16 calls).
Writes the table to --out (default profiles/scene_fit_cost.txt) and prints it.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PRECISION, SC, IMPORTANCE, G = "f16x3h", 64, 128, 128
STREAM_TBS = 6.2
AT_FLOOR_US = 3.0          # a call less than this above the floor of its launches is "at the floor"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scene_fit_cost.txt"))
    args = ap.parse_args()

    import torch
    from mc_nerf_amd import ops, synthetic as S
    from mc_nerf_amd.model import NeRF_Model

    dev = torch.device("cuda:0")
    N = args.rays
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def per_call_us(fn, calls=20):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3

    cube = (-3.5,) * 3 + (3.5,) * 3
    say(f"fitting the scene box to the voxel sigma cache: one MI355X, one process; reference rate {STREAM_TBS} TB/s (dw16_stream_kernel, profiles/r06_kernel_table_f16x3h.txt)")
    say()
    say("1. ops.voxel_box on its own (20 calls between two HIP events; three launches per call, the caller's own cells / box buffers)")
    cells, box = torch.empty(8, dtype=torch.int32, device=dev), torch.empty(6, device=dev)
    tiny = ops.VoxelGrid(2, -3.5, 3.5, -1.0, dev)
    floor = per_call_us(lambda: ops.voxel_box(tiny, 0.0, 2, cube, cells, box))
    say(f"  G =   2 (8 cells): {floor:8.1f} us per call: the floor of the three launches")
    for g_ in (128, 256, 384):
        grid = ops.VoxelGrid(g_, -3.5, 3.5, -1.0, dev)
        nbytes = 4 * g_ ** 3
        gen = torch.Generator(device=dev).manual_seed(g_)
        for name in ("no cell occupied", "1 % occupied", "every cell occupied"):
            if name == "1 % occupied":
                grid.vox.copy_(torch.where(torch.rand(g_, g_, g_, device=dev, generator=gen) < 0.01, torch.tensor(1.0, device=dev), torch.tensor(-1.0, device=dev)))
            elif name == "every cell occupied":
                grid.vox.fill_(1.0)
            us = per_call_us(lambda: ops.voxel_box(grid, 0.0, 2, cube, cells, box))
            pass_us = us - floor                            # (no rate is formed from a difference the size of the floor's own scatter)
            rest = f"less the floor {pass_us:8.1f} us = {nbytes / pass_us / 1e6:5.2f} TB/s" if pass_us >= AT_FLOOR_US else "at the floor"
            say(f"  G = {g_:3d} ({nbytes / 1e6:6.1f} MB), {name:20s} {us:8.1f} us per call = {nbytes / us / 1e6:5.2f} TB/s ({nbytes / us / 1e6 / STREAM_TBS:4.2f} of the reference); "
                f"{rest}; status {int(cells[6])}")
        del grid
        torch.cuda.empty_cache()

    say()
    say(f"2. ops.ray_depths, {N} rays, {SC} + {2 * SC} depths (20 calls between two HIP events; the wrapper's allocations included)")
    g = torch.Generator(device=dev).manual_seed(0)
    o = (4.0 * torch.nn.functional.normalize(torch.randn(N, 3, device=dev, generator=g), dim=-1)).contiguous()
    d = torch.nn.functional.normalize(1.2 * torch.randn(N, 3, device=dev, generator=g) - o, dim=-1).contiguous()
    gt = torch.rand(N, 3, device=dev, generator=g)
    zc, zf = torch.linspace(1.0, 8.0, SC, device=dev), torch.linspace(1.0, 8.0, 2 * SC, device=dev)
    jit = torch.rand(N, device=dev, generator=g) * 7.0 / SC
    six = (-1.2, -1.0, -1.4, 1.2, 1.0, 1.4)
    six_d = torch.tensor(six, device=dev)
    for name, fn in {"tuple (bounds library)": lambda: ops.ray_depths(o, d, six, 1.0, 8.0, jit, zc, zf),
                     "device box (fit library)": lambda: ops.ray_depths(o, d, six_d, 1.0, 8.0, jit, zc, zf),
                     "tuple with hit (hit library)": lambda: ops.ray_depths(o, d, six, 1.0, 8.0, jit, zc, zf, want_hit=True),
                     "device box with hit (fit library)": lambda: ops.ray_depths(o, d, six_d, 1.0, 8.0, jit, zc, zf, want_hit=True)}.items():
        say(f"  {name:36s} {per_call_us(fn):9.1f} us")

    say()
    say(f"3. render_rays_train + MSE loss + backward: {N} rays x ({SC} + {2 * SC}) samples (pdf: {SC} + {IMPORTANCE}), coarse 4x128, fine 8x256, {PRECISION}, voxel mode "
        f"(G = {G}, fresh grid), the cube as the box; {args.steps} steps per window after {args.warmup} warm-up steps, three alternating windows per mode")

    def make(fit, **kw):
        torch.manual_seed(42)
        sp = S.make_sys_param(dev, samples=SC, scale=2, batch=N, H=800, W=800, barf_mask=False, precision=PRECISION, ray_bounds="aabb",
                              ray_bounds_fit=fit, coarse_sampler="voxel", grid_nerf=G, voxel_warmup_epoch=0, voxel_beta=1e-6, **kw)
        m = NeRF_Model(sp).to(dev)
        m.reserve_workspaces(N)
        return m

    def train_step(m):
        def step(i):
            for p in m.parameters():
                p.grad = None
            rgb_c, rgb_f = m.render_rays_train(d, o, 20, 0.6)
            (((rgb_c - gt) ** 2).mean() + ((rgb_f - gt) ** 2).mean()).backward()
        return step

    def window(fn):
        for i in range(args.warmup):
            fn(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            fn(args.warmup + i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for fine in ("threshold", "pdf"):
        for miss in ("sample", "skip"):
            models = {fit: make(fit, fine_sampler=fine, n_importance=IMPORTANCE, ray_bounds_miss=miss) for fit in ("fixed", "voxel")}
            steps = {fit: train_step(m) for fit, m in models.items()}
            ms = {"fixed": [], "voxel": []}
            for _ in range(3):
                for fit in ("fixed", "voxel"):
                    ms[fit].append(window(steps[fit]))
            m = models["voxel"]
            same = m.scene_box.tolist() == list(m.settings.box) and m.settings.box == models["fixed"].settings.box
            fmt = lambda v: " ".join(f"{x:7.3f}" for x in v)
            say(f"  {fine:9s} / {miss:6s}  fixed {fmt(ms['fixed'])}   voxel {fmt(ms['voxel'])} ms   voxel - fixed = {min(ms['voxel']) - max(ms['fixed']):+.3f} .. "
                f"{max(ms['voxel']) - min(ms['fixed']):+.3f} ms   fits {(m._fit_calls + 15) // 16} in {m._fit_calls} calls, status {m.scene_box_status()}, the fitted box is the fixed one: {same}")
            del models, steps
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
