#!/usr/bin/env python3
"""Step time of the bench-shaped render with `ray_bounds_miss = "skip"` against "sample" (DESIGN.md 4l).

    python scripts/time_ray_skip.py [--steps K] [--warmup W] [--rays R] [--out FILE]

One MI355X, one process.  The nets of bench.py's default line (coarse 4x128 with 64 samples, fine 8x256 with 128; pdf mode: 64 + 128
depths), f16x3h, R = 32768 rays of cameras at radius 4 looking at points within 1.2 of the origin.  The box is a centred cube whose half
size is searched so that about 0, 1/3 and 2/3 of those rays miss it (share 0: the cube +-1e3, which every ray crosses over all of
[near, far]).  A step is NeRF_Model.render_rays_train on those rays, an MSE loss on both colours and the backward -- the part of the
train step the key changes; "sample" on this build is the parent commit's aabb path launch for launch.  Timed in this order:
  1. per sampler pair (threshold / pdf x dense / voxel) and miss share: "sample" and "skip" in three alternating windows.  The spread of
     the windows of one mode is the margin a difference must exceed to be called one; at share 0 both modes evaluate the same samples,
     so their difference is the feature's overhead (the flags, the two lists, the listed instead of the dense MLP launches).  In voxel
     mode the grid is fresh (every cell occupied: the list is every pair of the rays that hit) and voxel_beta is 1e-6;
  2. the no-grad render (render_rays_test), threshold / dense, at each share;
  3. the new launches on their own beside the ones they replace (20 calls between two HIP events).
Writes the table to --out (default profiles/ray_skip_cost.txt) and prints it.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PRECISION, SC, IMPORTANCE, G = "f16x3h", 64, 128, 128
SHARES = (0.0, 1.0 / 3.0, 2.0 / 3.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ray_skip_cost.txt"))
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

    g = torch.Generator(device=dev).manual_seed(0)
    o = (4.0 * torch.nn.functional.normalize(torch.randn(N, 3, device=dev, generator=g), dim=-1)).contiguous()
    d = torch.nn.functional.normalize(1.2 * torch.randn(N, 3, device=dev, generator=g) - o, dim=-1).contiguous()
    gt = torch.rand(N, 3, device=dev, generator=g)
    zgrid = torch.linspace(1.0, 8.0, SC, device=dev)

    def miss_share(half):
        hit = ops.ray_depths(o, d, (-half,) * 3 + (half,) * 3, 1.0, 8.0, None, zgrid, want_span=False, want_hit=True)[3]
        return float((hit == 0).float().mean())

    def box_for(share):
        if share == 0.0:
            return 1e3
        lo, hi = 0.01, 8.0                                  # the share falls as the cube grows
        for _ in range(30):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if miss_share(mid) > share else (lo, mid)
        return hi

    def make(half, miss, **kw):
        torch.manual_seed(42)
        sp = S.make_sys_param(dev, samples=SC, scale=2, batch=N, H=800, W=800, barf_mask=False, precision=PRECISION, ray_bounds="aabb",
                              ray_bounds_box=(-half,) * 3 + (half,) * 3, ray_bounds_miss=miss, **kw)
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

    def render_step(m):
        def step(i):
            m.render_rays_test(d, o, m.nerf_coarse, m.nerf_fine)
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

    def compare(label, half, stepper, **kw):
        models = {miss: make(half, miss, **kw) for miss in ("sample", "skip")}
        steps = {miss: stepper(m) for miss, m in models.items()}
        ms = {"sample": [], "skip": []}
        for _ in range(3):
            for miss in ("sample", "skip"):
                ms[miss].append(window(steps[miss]))
        nerf = models["skip"]
        share = float((nerf.last_ray_hit == 0).float().mean())
        lists = []
        for sel, rows in ((nerf.last_coarse_selection, N * SC), (nerf.last_selection, nerf.settings.fine_rows(N, train=False))):
            lists.append(int(sel[1].item()) / rows)
        fmt = lambda v: " ".join(f"{x:7.3f}" for x in v)
        say(f"{label:34s} miss {share:5.3f}   sample {fmt(ms['sample'])}   skip {fmt(ms['skip'])} ms   sample - skip = {min(ms['sample']) - max(ms['skip']):+.3f} .. "
            f"{max(ms['sample']) - min(ms['skip']):+.3f} ms   lists {lists[0]:.3f} of N Sc, {lists[1]:.3f} of the fine rows")
        del models, steps
        torch.cuda.empty_cache()

    say(f"skipping the rays that miss the box: {N} rays x ({SC} + {2 * SC}) samples (pdf: {SC} + {IMPORTANCE}), coarse 4x128, fine 8x256, {PRECISION}, "
        f"{args.steps} steps per window after {args.warmup} warm-up steps, three alternating windows per mode, one process")
    halves = {share: box_for(share) for share in SHARES}
    say("centred cube, half size -> miss share: " + ", ".join(f"{h:.4g} -> {miss_share(h):.3f}" for h in halves.values()))
    say()
    say("1. render_rays_train + MSE loss + backward")
    for fine in ("threshold", "pdf"):
        for coarse in ("dense", "voxel"):
            kw = dict(fine_sampler=fine, n_importance=IMPORTANCE)
            if coarse == "voxel":
                kw.update(coarse_sampler="voxel", grid_nerf=G, voxel_warmup_epoch=0, voxel_beta=1e-6)
            for share in SHARES:
                compare(f"{fine} / {coarse}", halves[share], train_step, **kw)
    say()
    say("2. render_rays_test (no grad), threshold / dense")
    for share in SHARES:
        compare("render", halves[share], render_step)
    say()
    say("3. the launches on their own (20 calls between two HIP events; the wrapper's allocations included), at miss share 1/3")
    half = halves[SHARES[1]]
    box = (-half,) * 3 + (half,) * 3
    zf = torch.linspace(1.0, 8.0, 2 * SC, device=dev)
    jit = torch.rand(N, device=dev, generator=g) * 7.0 / SC
    z_c, _, _, hit = ops.ray_depths(o, d, box, 1.0, 8.0, jit, zgrid, zf, want_hit=True)
    w = torch.rand(N, SC, device=dev, generator=g) ** 6
    wmax = w.max().reshape(1).view(torch.int32)
    grid = ops.VoxelGrid(G, -3.5, 3.5, 30.0, dev)
    fns = {"ray_depths (bounds library)": lambda: ops.ray_depths(o, d, box, 1.0, 8.0, jit, zgrid, zf),
           "ray_depths with hit": lambda: ops.ray_depths(o, d, box, 1.0, 8.0, jit, zgrid, zf, want_hit=True),
           f"list_rays, S = {SC}": lambda: ops.list_rays(hit, SC, -20.0),
           f"list_rays, S = {SC + IMPORTANCE}": lambda: ops.list_rays(hit, SC + IMPORTANCE, -20.0),
           "select_fine (core library)": lambda: ops.select_fine(w, wmax, 0.5, 2, -20.0),
           "select_fine behind the flag": lambda: ops.select_fine(w, wmax, 0.5, 2, -20.0, hit=hit),
           "voxel_select on rows (bounds library)": lambda: ops.voxel_select(grid, 0.0, o, d, None, None, -20.0, z_rows=z_c),
           "voxel_select on rows behind the flag": lambda: ops.voxel_select(grid, 0.0, o, d, None, None, -20.0, z_rows=z_c, hit=hit)}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        say(f"  {name:40s} {e0.elapsed_time(e1) / 20 * 1e3:9.1f} us")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
