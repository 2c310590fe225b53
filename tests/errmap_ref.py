"""Torch restatement of the error-guided pixel sampler (csrc/errmap.hip) on host tensors: int64 tile weights, cumsum,
searchsorted(right=True); fp32 for the in-tile index and for the per-ray error; the blend with separately rounded fp32 products.
Every quantity is formed in the kernel's number format by one IEEE operation at a time, so the tests demand equality."""
import torch

ONE_BELOW = float(torch.tensor(1.0) - torch.tensor(2.0 ** -24))       # 1 - 2^-24, the largest fp32 below 1
THIRD = torch.tensor(0.333333343, dtype=torch.float32)


def f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def tiles(H, W, tile):
    """-> Th, Tw, th [Th*Tw], tw [Th*Tw] (int64): rows and columns of every tile, row-major; edge tiles are smaller."""
    Th, Tw = -(-H // tile), -(-W // tile)
    th = torch.clamp(H - torch.arange(Th) * tile, max=tile)
    tw = torch.clamp(W - torch.arange(Tw) * tile, max=tile)
    return Th, Tw, th[:, None].expand(Th, Tw).reshape(-1).contiguous(), tw[None, :].expand(Th, Tw).reshape(-1).contiguous()


def weights(E, H, W, tile):
    """E [Th,Tw] fp32 -> q [Th*Tw] int64 = max(1, trunc(clamp(E, 0, 4) * 2^24)) * area (NaN -> 0, +inf -> 4)."""
    Th, Tw, th, tw = tiles(H, W, tile)
    e = E.reshape(-1).float()
    c = torch.where(torch.isnan(e), torch.zeros_like(e), e).clamp(0.0, 4.0)
    return (c * 16777216.0).to(torch.int64).clamp(min=1) * (th * tw)


def unit(u):
    """fminf(fmaxf(u, 0), 1 - 2^-24); NaN -> 0."""
    u = u.float()
    return torch.where(torch.isnan(u), torch.zeros_like(u), u).clamp(0.0, ONE_BELOW)


def sample(err, H, W, tile, seg_cam, seg_start, uniform_frac, u):
    """err [C,Th,Tw], u [n,2] -> pix [n] int64."""
    Th, Tw, th, tw = tiles(H, W, tile)
    T, npix = Th * Tw, H * W
    frac = f32(uniform_frac)
    u = unit(u.reshape(-1, 2))
    out = torch.empty(int(seg_start[-1]), dtype=torch.int64)
    for k, cam in enumerate(seg_cam):
        a, b = int(seg_start[k]), int(seg_start[k + 1])
        if b == a:
            continue
        n_u = int(frac * (b - a))
        u0, u1 = u[a:b, 0], u[a:b, 1]
        uni = (u0.double() * float(npix)).to(torch.int64).clamp(max=npix - 1)
        cdf = torch.cumsum(weights(err[cam], H, W, tile), 0)
        target = (u0.double() * float(int(cdf[-1]))).to(torch.int64)
        assert bool((target < cdf[-1]).all())
        t = torch.searchsorted(cdf, target, right=True).clamp(max=T - 1)
        ty, tx = t // Tw, t % Tw
        area = th[t] * tw[t]
        l = torch.minimum((u1 * area.float()).to(torch.int64), area - 1)
        epix = (ty * tile + l // tw[t]) * W + tx * tile + l % tw[t]
        j = torch.arange(b - a)
        out[a:b] = torch.where(j < n_u, uni, epix)
    return out


def ray_error(rgb, gt):
    """((d0^2 + d1^2) + d2^2) * fp32(1/3), every step rounded to fp32."""
    d = rgb.float() - gt.float()
    sq = d * d
    return ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) * THIRD


def update(err, H, W, tile, seg_cam, seg_start, pix, rgb, gt, beta):
    """-> the new map [C,Th,Tw] (err is left as it is): per touched tile E <- (1 - beta) E + beta max(e), products rounded apart."""
    Th, Tw, _, _ = tiles(H, W, tile)
    b32 = torch.tensor(float(beta), dtype=torch.float32)
    omb = torch.tensor(1.0, dtype=torch.float32) - b32
    out = err.clone().float()
    flat = out.view(-1)
    e = ray_error(rgb, gt)
    best = {}
    for k, cam in enumerate(seg_cam):
        for i in range(int(seg_start[k]), int(seg_start[k + 1])):
            p = int(pix[i])
            if p < 0 or p >= H * W or not bool(torch.isfinite(e[i])):
                continue
            cell = (cam * Th + (p // W) // tile) * Tw + (p % W) // tile
            best[cell] = e[i] if cell not in best else torch.maximum(best[cell], e[i])
    for cell, m in best.items():
        flat[cell] = omb * flat[cell] + b32 * m
    return out


def tile_of(pix, W, tile, Tw):
    return (pix // W) // tile * Tw + (pix % W) // tile
