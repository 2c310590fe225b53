"""Shapes, gradient schedules and runners shared by tests/test_radam_rows_cpu.py and tests/test_radam_rows_gpu.py (the row-lazy RAdam
of DESIGN.md 4g).

The shapes: (110, 6) and (110,) are the camera tensors at the rig's 110 cameras; (7, 2) and (1, 6) leave a block of four rows partly
empty; (65, 1) is rows of one element over more than one block per 64 rows; in (3, 130) a row is longer than a wave and ragged in its
third pass (130 = 64 + 64 + 2).

The sparse schedule, per tensor of R rows and per step:
  * every row but two is visited with probability 1/2 (a random subset per step and tensor);
  * row 0 is visited on every step (it crosses t = 6, the N_sma >= 5 switch at beta2 = 0.999; most rows never do);
  * row R - 1 (R > 1) is never visited;
  * step ZERO_STEP visits nothing, in any tensor;
  * step 2: row 1 % R holds zeros and one non-zero in its LAST element;
  * step 3: row 2 % R holds only -0.0 (not a visit);
  * step 4: row 3 % R holds zeros and one denormal (a visit).
"""
import torch

SHAPES = [(110, 6), (110,), (7, 2), (1, 6), (65, 1), (3, 130)]
STEPS = 12
ZERO_STEP = 5
HYPER = dict(lr=3e-3, betas=(0.9, 0.999), weight_decay=4e-4)
DENORMAL = 1e-40


def rows_of(t):
    return t.reshape(t.shape[0], -1)


def visited(g):
    """The rule itself: the rows with an element != 0."""
    return (rows_of(g) != 0).any(dim=1)


def params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen) for s in SHAPES]


def sparse_schedule(steps=STEPS, seed=1):
    """-> grads[step][tensor], CPU fp32."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for step in range(steps):
        gs = []
        for shape in SHAPES:
            R = shape[0]
            g = torch.randn(shape, generator=gen)
            keep = torch.rand(R, generator=gen) < 0.5
            keep[0] = True
            if R > 1:
                keep[R - 1] = False
            if step == ZERO_STEP:
                keep[:] = False
            g2 = rows_of(g)
            g2[~keep] = 0.0
            if step == 2:
                r = 1 % R
                last = g2[r, -1].clone() if float(g2[r, -1]) != 0.0 else torch.tensor(0.37)
                g2[r] = 0.0
                g2[r, -1] = last
            if step == 3:
                g2[2 % R] = -0.0
            if step == 4:
                assert R == 1 or 3 % R != R - 1
                g2[3 % R] = 0.0
                g2[3 % R, 0] = DENORMAL
            gs.append(g)
        out.append(gs)
    return out


def dense_schedule(steps=9, seed=2):
    gen = torch.Generator().manual_seed(seed)
    out = [[torch.randn(s, generator=gen) for s in SHAPES] for _ in range(steps)]
    assert all(bool(visited(g).all()) for gs in out for g in gs)
    return out


def snapshot(opt, ps):
    """-> per tensor (p, exp_avg, exp_avg_sq, row_step | None), cloned."""
    out = []
    for p in ps:
        st = opt.state[p]
        rs = st.get("row_step")
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), None if rs is None else rs.clone()))
    return out


def run(ps0, schedule, dev, lazy, each_step=False, **kw):
    """RAdam over clones of `ps0` on `dev`, one group (lazy or dense), through `schedule` -> (optimiser, parameters, snapshots): the
    snapshot after the last step, or with `each_step` the list of the snapshots after every step."""
    from mc_nerf_amd.model import RAdam
    ps = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ps0]
    opt = RAdam([{"params": ps, "lazy_rows": lazy}], **{**HYPER, **kw})
    snaps = []
    for gs in schedule:
        for p, g in zip(ps, gs):
            p.grad = g.to(dev)
        opt.step()
        if each_step:
            snaps.append(snapshot(opt, ps))
    return opt, ps, (snaps if each_step else snapshot(opt, ps))


def per_row_dense(ps0, schedule, dev, **kw):
    """The independence reference: for every row of every tensor a DENSE RAdam of its own on a single-row clone, stepped only on the
    steps that visit the row -> per tensor (p, exp_avg, exp_avg_sq, row_step) assembled from the rows."""
    from mc_nerf_amd.model import RAdam
    out = []
    for ti, p0 in enumerate(ps0):
        R = p0.shape[0]
        rows = [torch.nn.Parameter(p0[r:r + 1].detach().clone().to(dev)) for r in range(R)]
        opts = [RAdam([row], **{**HYPER, **kw}) for row in rows]
        counts = torch.zeros(R, dtype=torch.int32)
        for gs in schedule:
            g = gs[ti]
            vis = visited(g)
            for r in vis.nonzero().flatten().tolist():
                rows[r].grad = g[r:r + 1].to(dev)
                opts[r].step()
                counts[r] += 1
        zero = lambda row: torch.zeros_like(row.detach())
        m = [o.state[row]["exp_avg"] if o.state[row] else zero(row) for o, row in zip(opts, rows)]
        v = [o.state[row]["exp_avg_sq"] if o.state[row] else zero(row) for o, row in zip(opts, rows)]
        out.append((torch.cat([row.detach() for row in rows]), torch.cat(m), torch.cat(v), counts.to(dev)))
    return out


def same_bits(a, b):
    """torch.equal, but on the bits where it matters: -0.0 and 0.0 differ, NaN equals itself."""
    if a.dtype.is_floating_point:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)
