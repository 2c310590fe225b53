"""The voxel sigma cache restated in plain torch on the CPU (include/mcnerf.h: mcnerf_voxel_*; csrc/voxel.hip): the cell of a point,
the coarse (ray, sample) list, the update rule and the centre grid, exactly as the kernels define them -- every step a separately
rounded fp32 operation, so the device results are compared with torch.equal, not with a tolerance."""
import torch

F32 = torch.float32


def _f32(x):
    return torch.tensor(float(x), dtype=F32)


def scale_of(G, bmin, bmax):
    """s = float32(G) / float32(bmax - bmin): one fp32 division."""
    return _f32(G) / _f32(float(bmax) - float(bmin))


def cell_axis(p, G, bmin, bmax):
    t = (p.to(F32) - _f32(bmin)) * scale_of(G, bmin, bmax)
    t = torch.where(torch.isnan(t), torch.zeros_like(t), t)             # fmaxf(NaN, 0) = 0
    return torch.clamp(t, 0.0, float(G - 1)).to(torch.int64)            # (int) truncation of a value in [0, G - 1]


def cell_of(xyz, G, bmin, bmax):
    """xyz [..., 3] -> linear cell index (ix * G + iy) * G + iz, int64."""
    i = cell_axis(xyz, G, bmin, bmax)
    return (i[..., 0] * G + i[..., 1]) * G + i[..., 2]


def sample_points(rays_o, rays_d, zgrid, jitter):
    """p[n, j] = o[n] + d[n] * (zgrid[j] + jitter[n]), [N,Sc,3]; each multiply and add rounded to fp32 on its own."""
    z = zgrid.to(F32).unsqueeze(0).expand(rays_d.shape[0], -1)
    if jitter is not None:
        z = z + jitter.to(F32).reshape(-1, 1)
    return rays_o.to(F32).unsqueeze(1) + rays_d.to(F32).unsqueeze(1) * z.unsqueeze(2)


def sample_cells(rays_o, rays_d, zgrid, jitter, G, bmin, bmax):
    return cell_of(sample_points(rays_o, rays_d, zgrid, jitter), G, bmin, bmax)


def select(vox, thresh, rays_o, rays_d, zgrid, jitter, bmin, bmax, sigma_default):
    """-> idx [K,2] int64 in torch.nonzero (row-major) order, out_c [N,Sc,4] = (sigma_default, 1, 1, 1)."""
    G = vox.shape[0]
    cells = sample_cells(rays_o, rays_d, zgrid, jitter, G, bmin, bmax)
    idx = torch.nonzero(vox.reshape(-1)[cells] > _f32(thresh))
    out_c = torch.ones(*cells.shape, 4, dtype=F32)
    out_c[..., 0] = float(sigma_default)
    return idx, out_c


def _key(sig):
    """The order-preserving uint32 key of a float (held in int64): a < b <=> key(a) < key(b); every finite float's key is > 0."""
    u = sig.to(F32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def _unkey(k):
    u = torch.where(k >= 0x80000000, k & 0x7FFFFFFF, 0xFFFFFFFF - k)
    return torch.where(u >= 0x80000000, u - (1 << 32), u).to(torch.int32).view(F32)


def update_cells(vox, cells, sigma, beta):
    """The update rule on (cell, sigma) items -> the new grid (a copy): per touched cell m = max of the finite sigmas,
    V <- fadd(fmul(1 - beta, V), fmul(beta, m)) with 1 - beta formed in fp32; untouched cells keep their bits."""
    out = vox.clone().reshape(-1)
    cells, sigma = cells.reshape(-1), sigma.to(F32).reshape(-1)
    ok = torch.isfinite(sigma)
    cells, sigma = cells[ok], sigma[ok]
    if cells.numel() == 0:
        return out.reshape(vox.shape)
    keys = torch.zeros(out.numel(), dtype=torch.int64).scatter_reduce(0, cells, _key(sigma), "amax", include_self=True)
    touched = torch.nonzero(keys > 0).reshape(-1)
    b = _f32(beta)
    omb = _f32(1.0) - b
    out[touched] = omb * out[touched] + b * _unkey(keys[touched])
    return out.reshape(vox.shape)


def update(vox, beta, rays_o, rays_d, zgrid, jitter, sig, bmin, bmax, idx=None):
    """The update from ray samples: sig [N,Sc] raw sigma; idx [K,2] = the listed pairs, None = all N * Sc."""
    cells = sample_cells(rays_o, rays_d, zgrid, jitter, vox.shape[0], bmin, bmax)
    if idx is not None:
        r, j = idx[:, 0].long(), idx[:, 1].long()
        cells, sig = cells[r, j], sig[r, j]
    return update_cells(vox, cells, sig, beta)


def update_points(vox, xyz, sigma, beta, bmin, bmax):
    return update_cells(vox, cell_of(xyz, vox.shape[0], bmin, bmax), sigma, beta)


def query(vox, xyz, bmin, bmax):
    return vox.reshape(-1)[cell_of(xyz, vox.shape[0], bmin, bmax)]


def centres(G, bmin, bmax):
    """Cell centres bmin + (i + 1/2) (scope / G), [G,G,G,3] fp32."""
    axis = (torch.arange(G, dtype=F32) + 0.5) * _f32((float(bmax) - float(bmin)) / G) + _f32(bmin)
    return torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1)
