"""Per-ray sample bounds (`ray_bounds = "aabb"`; include/mcnerf_box.h, csrc/ray_bounds.hip) restated in plain torch on the CPU: every
step a separately rounded fp32 operation, fmin / fmax with C's NaN rule (torch.fmin / torch.fmax), so the device results are compared
with torch.equal.  Also the voxel cache's restatement (tests/voxel_ref.py) and the sampler's (tests/pdf_ref.py) on per-ray rows, and
the hand-made rays of the GPU tests."""
import torch

import voxel_ref as V
from pdf_ref import sample_pdf_ref

F32 = torch.float32
INF, NAN = float("inf"), float("nan")
NEAR, FAR = 1.0, 8.0
BOX = (-1.0, -1.5, -0.5, 1.0, 1.5, 2.0)                     # non-cubic, off-centre in z
NO_CLIP = (-1e3,) * 3 + (1e3,) * 3                          # a box that clips no ray of a scene within [near, far] of its cameras


def _f32(x):
    return torch.tensor(float(x), dtype=F32)


def span_ref(o, d, box, near, far):
    """-> lo [N], hi [N], clipped [N] bool."""
    o, d = o.to(F32), d.to(F32)
    bmin, bmax = torch.tensor(box[:3], dtype=F32), torch.tensor(box[3:], dtype=F32)
    near, far = _f32(near), _f32(far)
    t0, t1 = (bmin - o) / d, (bmax - o) / d
    nz = d != 0                                             # (NaN != 0: a NaN direction takes the division branch)
    miss = (nz & (torch.isnan(t0) | torch.isnan(t1))) | (~nz & ~((bmin <= o) & (o <= bmax)))
    lo_k = torch.where(nz, torch.fmin(t0, t1), torch.full_like(t0, -INF))
    hi_k = torch.where(nz, torch.fmax(t0, t1), torch.full_like(t0, INF))
    t_in = torch.fmax(torch.fmax(lo_k[:, 0], lo_k[:, 1]), lo_k[:, 2])
    t_out = torch.fmin(torch.fmin(hi_k[:, 0], hi_k[:, 1]), hi_k[:, 2])
    lo, hi = torch.fmax(near.expand_as(t_in), t_in), torch.fmin(far.expand_as(t_out), t_out)
    clipped = ~miss.any(-1) & torch.isfinite(lo) & torch.isfinite(hi) & (hi > lo)
    return torch.where(clipped, lo, near), torch.where(clipped, hi, far), clipped


def depths_ref(o, d, box, near, far, jitter, grid):
    """-> z [N,S] of `grid` [S], span [N,2], clipped [N]."""
    lo, hi, clipped = span_ref(o, d, box, near, far)
    a = (hi - lo) / (_f32(far) - _f32(near))
    b = lo - a * _f32(near)
    z = a.unsqueeze(1) * grid.to(F32).unsqueeze(0) + b.unsqueeze(1)
    if jitter is not None:
        z = z + (a * jitter.to(F32).reshape(-1)).unsqueeze(1)
    return z, torch.stack([lo, hi], -1), clipped


def depths_exact(span, near, far, jitter, grid):
    """The affine map in fp64 on the fp32 span: lo + (hi - lo) (g - near + jitter) / (far - near)."""
    lo, hi = span[:, :1].double(), span[:, 1:].double()
    t = grid.double().unsqueeze(0) - near + (0.0 if jitter is None else jitter.double().reshape(-1, 1))
    return lo + (hi - lo) * t / (far - near)


def affine_bound(far, max_jitter):
    """|z - depths_exact| of a row, from the roundings alone (u = 2^-24, the unit roundoff of fp32; second-order terms in the slack).
    z = lo + a (g - near + jitter) with 0 <= a <= 1 (hi - lo <= far - near), near >= 0 and lo in [near, far], so F = far + max jitter
    bounds every intermediate: |a g|, |a near|, b = lo - a near in [0, far], a g + b = lo + a (g - near) <= hi, |a jitter|, |z|.
      a        three roundings (hi - lo, far - near, the quotient): relative error 3 u, which moves z by 3 u a (g - near + jitter) <= 3 u F
      b        fl(a near) and the subtraction: 2 u F
      z        fl(a g), fl(. + b), fl(a jitter), the last sum: 4 u F
    9 u F in all; 10 u F with the slack."""
    return 10.0 * 2.0 ** -24 * (far + max_jitter)


def points_rows(o, d, rows):
    """p[n, j] = o[n] + d[n] * rows[n, j], [N,S,3]; each multiply and add rounded to fp32 on its own."""
    return o.to(F32).unsqueeze(1) + d.to(F32).unsqueeze(1) * rows.to(F32).unsqueeze(2)


def cells_rows(o, d, rows, G, bmin, bmax):
    return V.cell_of(points_rows(o, d, rows), G, bmin, bmax)


def select_rows(vox, thresh, o, d, rows, bmin, bmax, sigma_default):
    """tests/voxel_ref.py::select on per-ray rows."""
    cells = cells_rows(o, d, rows, vox.shape[0], bmin, bmax)
    idx = torch.nonzero(vox.reshape(-1)[cells] > _f32(thresh))
    out_c = torch.ones(*cells.shape, 4, dtype=F32)
    out_c[..., 0] = float(sigma_default)
    return idx, out_c


def update_rows(vox, beta, o, d, rows, sig, bmin, bmax, idx=None):
    """tests/voxel_ref.py::update on per-ray rows."""
    cells = cells_rows(o, d, rows, vox.shape[0], bmin, bmax)
    if idx is not None:
        r, j = idx[:, 0].long(), idx[:, 1].long()
        cells, sig = cells[r, j], sig[r, j]
    return V.update_cells(vox, cells, sig, beta)


def sample_pdf_rows_ref(w, rows, u):
    """tests/pdf_ref.py::sample_pdf_ref ray by ray (it takes one grid per call: the ray's own row) -> (z_all, zs, zc) as it returns them."""
    parts = [sample_pdf_ref(w[n:n + 1], rows[n], None, u[n:n + 1]) for n in range(w.shape[0])]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3))


# ---- the rays of the GPU tests: (origin, direction, clipped by BOX on [NEAR, FAR]?)
HAND = [
    ((-4.0, 0.2, 0.1), (0.99, 0.1, 0.05), True),            # a hit from outside
    ((0.0, 0.0, 0.0), (0.6, 0.64, 0.48), True),             # origin inside the box: lo = near
    ((-4.0, 5.0, 0.0), (0.99, 0.1, 0.1), False),            # a miss
    ((-4.0, 0.2, 0.1), (1.0, 0.1, 0.0), True),              # one zero component, inside its slab
    ((-4.0, 0.2, 0.1), (1.0, 0.1, -0.0), True),             # ... as -0.0
    ((-4.0, 0.2, 3.0), (1.0, 0.1, 0.0), False),             # ... outside its slab
    ((-4.0, 0.2, -3.0), (1.0, 0.1, -0.0), False),
    ((-4.0, 0.0, 0.5), (1.0, 0.0, -0.0), True),             # two zero components, inside
    ((-4.0, 2.0, 0.5), (1.0, -0.0, 0.0), False),            # ... one of them outside
    ((0.0, 0.0, 0.0), (0.0, -0.0, 0.0), True),              # three zero components inside: unconstrained, (near, far)
    ((5.0, 5.0, 5.0), (0.0, 0.0, 0.0), False),              # ... outside
    ((-4.0, -1.5, 0.0), (1.0, 0.0, 0.0), True),             # along a face: o == min with d == 0
    ((-4.0, 1.5, 2.0), (1.0, 0.0, 0.0), True),              # along an edge: o == max on two axes
    ((-3.0, -0.5, 0.0), (1.0, 1.0, 0.0), False),            # a corner graze: t_in == t_out == 2, hi == lo
    ((-20.0, 0.1, 0.1), (1.0, 0.0, 0.0), False),            # the box beyond far
    ((0.5, 0.0, 0.0), (1.0, 0.0, 0.0), False),              # the box nearer than near: t_out = 0.5
    ((-1.2, 0.0, 0.0), (1.0, 0.0, 0.0), True),              # ... partly: [0.2, 2.2] -> [1, 2.2]
    ((NAN, 0.0, 0.0), (1.0, 0.0, 0.0), False),
    ((-4.0, 0.0, 0.0), (1.0, NAN, 0.0), False),
    ((0.0, 0.0, 0.0), (NAN, 0.6, 0.8), False),
    ((INF, 0.0, 0.0), (-1.0, 0.0, 0.0), False),
    ((-INF, 0.0, 0.0), (1.0, 0.1, 0.0), False),
    ((-4.0, 0.0, 0.0), (INF, 0.0, 0.0), False),
    ((-4.0, 0.0, 0.0), (1.0, -INF, 0.0), False),
    ((INF, 0.0, 0.0), (INF, 0.0, 0.0), False),              # inf - inf, inf / inf
    ((3e38, 0.0, 0.0), (-INF, 0.0, 0.0), False),            # finite / inf = 0 on both ends: the interval [0, 0]
]


def camera_rays(N, seed, radius=4.0, spread=1.0):
    """Rays of cameras on a sphere of `radius` looking at points within `spread` of the origin (unit directions)."""
    g = torch.Generator().manual_seed(seed)
    o = radius * torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    d = torch.nn.functional.normalize(spread * torch.randn(N, 3, generator=g) - o, dim=-1)
    return d, o, g


def hand_rays(N, seed=11):
    """-> o [N,3], d [N,3]: the hand-made rays first, then camera rays (a part of which miss BOX)."""
    d_r, o_r, _ = camera_rays(max(N - len(HAND), 0), seed, spread=1.6)
    o = torch.cat([torch.tensor([h[0] for h in HAND], dtype=F32), o_r])[:N]
    d = torch.cat([torch.tensor([h[1] for h in HAND], dtype=F32), d_r])[:N]
    return o.contiguous(), d.contiguous()


def model_rays(N, seed=5):
    """-> d, o of the GPU model tests: between 1/2 and 9/10 of them are clipped by BOX and at least one misses it
    (tests/test_ray_bounds_cpu.py asserts both)."""
    d, o, _ = camera_rays(N, seed, spread=1.2)
    return d.contiguous(), o.contiguous()
