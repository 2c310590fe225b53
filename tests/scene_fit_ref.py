"""The scene box fitted to the voxel sigma cache (`ray_bounds_fit = "voxel"`; include/mcnerf_fit.h, csrc/scene_fit.hip) restated in plain
torch on the CPU: the occupied cells' index range, its padding, the two fp32 bounds per axis (a multiply and an add, each rounded on its
own), the clamp to the outer box with C's fmaxf / fminf (torch.fmax / torch.fmin) and the status.  The device results are compared with
torch.equal.  Also the hand-made grids of the tests."""
import torch

F32 = torch.float32
INF, NAN = float("inf"), float("nan")


def _f32(x):
    return torch.tensor(float(x), dtype=F32)


def cell_edge(G, bmin, bmax):
    """h = float32(bmax - bmin) / float32(G): what the host hands to the kernel."""
    return float(_f32(float(bmax) - float(bmin)) / _f32(G))


def voxel_box_ref(vox, bmin, h, thresh, margin, outer):
    """vox [G,G,G] fp32, the cube's corner, the cell edge (fp32 values), margin >= 0, outer = (xmin, ymin, zmin, xmax, ymax, zmax)
    -> cells [8] int32 = (i0x, i0y, i0z, i1x, i1y, i1z, status, 0), box [6] fp32."""
    G = vox.shape[0]
    assert tuple(vox.shape) == (G, G, G) and vox.dtype == F32
    outer_t = torch.tensor([float(v) for v in outer], dtype=F32)
    occ = torch.nonzero(vox > _f32(thresh))                 # [M,3]: (ix, iy, iz); NaN > t and t > t are False, +inf > t is True
    if occ.shape[0] == 0:
        return torch.tensor([G, G, G, -1, -1, -1, 0, 0], dtype=torch.int32), outer_t
    i0, i1 = occ.min(0).values, occ.max(0).values
    j0, j1 = (i0 - margin).clamp(min=0), (i1 + margin).clamp(max=G - 1)
    lo = _f32(bmin) + j0.to(F32) * _f32(h)
    hi = _f32(bmin) + (j1 + 1).to(F32) * _f32(h)
    lo, hi = torch.fmax(lo, outer_t[:3]), torch.fmin(hi, outer_t[3:])
    ok = bool((lo < hi).all())
    cells = torch.cat([i0, i1, torch.tensor([1 if ok else 2, 0])]).to(torch.int32)
    return cells, torch.cat([lo, hi]) if ok else outer_t


def box_of_cells(j0, j1, bmin, h):
    """The fp32 bounds of the cell range j0 .. j1 (three indices each) without an outer box, as six Python floats."""
    lo = [float(_f32(bmin) + _f32(j) * _f32(h)) for j in j0]
    hi = [float(_f32(bmin) + _f32(j + 1) * _f32(h)) for j in j1]
    return tuple(lo + hi)


# ---- the grids of the tests: `below` everywhere but in the cells named
def grid_with(G, cells, value=1.0, below=-1.0):
    vox = torch.full((G, G, G), float(below), dtype=F32)
    for c in cells:
        vox[tuple(c[:3])] = float(value) if len(c) == 3 else float(c[3])     # (a fourth entry: that cell's own value)
    return vox


def corners(G):
    return [(x, y, z) for x in (0, G - 1) for y in (0, G - 1) for z in (0, G - 1)]


def random_fill(G, share, seed, below=-1.0):
    """A share of the cells at U(0.5, 1.5) above a threshold of 0, the rest at `below`."""
    g = torch.Generator().manual_seed(seed)
    on = torch.rand(G, G, G, generator=g) < share
    return torch.where(on, torch.rand(G, G, G, generator=g) + 0.5, torch.tensor(float(below)))


def blob(G, lo, hi, value=5.0, below=-5.0):
    """Every cell of the index range lo .. hi (three indices each, inclusive) at `value`, the rest at `below`."""
    vox = torch.full((G, G, G), float(below), dtype=F32)
    vox[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = float(value)
    return vox
