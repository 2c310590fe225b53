"""Skipping the rays that miss the scene box (`ray_bounds_miss = "skip"`; include/mcnerf_hit.h, csrc/ray_skip.hip) restated in plain torch
on the CPU, from the restatements of what it gates: the flag is `ray_bounds_ref.span_ref`'s third result, the fine selection is
`oracle.select_fine`'s rule, the voxel list `ray_bounds_ref.select_rows`.  Lists are [K,2] int64 in torch.nonzero order and are compared
exactly."""
import torch

import ray_bounds_ref as B
from oracle import mcnerf_oracle as O

F32 = torch.float32


def hit_ref(o, d, box, near, far):
    """-> hit [N] int32: 1 iff the box clips the ray (the rule: include/mcnerf_box.h)."""
    return B.span_ref(o, d, box, near, far)[2].to(torch.int32)


def prefill_ref(N, S, sigma_default):
    out = torch.ones(N, S, 4, dtype=F32)
    out[..., 0] = float(sigma_default)
    return out


def list_rays_ref(hit, S, sigma_default):
    """-> idx [S * #hit, 2], out [N,S,4]: every (n, j), j < S, of the rays with hit[n] != 0, and the prefill of all rays."""
    mask = (hit != 0).unsqueeze(1).expand(-1, S)
    return torch.nonzero(mask), prefill_ref(hit.shape[0], S, sigma_default)


def filter_by_ray(idx, hit):
    """The entries of a list whose ray has hit != 0, in the list's order."""
    return idx[(hit != 0)[idx[:, 0].long()]]


def select_fine_ref(w_sel, wmax, thresh, scale, sigma_default, hit):
    """oracle.select_fine's rule behind the flag: (n, j) contributes its `scale` fine samples (n, j * scale + r) iff hit[n] != 0 and
    w_sel[n,j] >= min(thresh, wmax), `wmax` being the composite's own maximum over ALL rays.  A masked ray's weights never reach a
    comparison (they may be NaN)."""
    N, Sc = w_sel.shape
    thr = torch.minimum(torch.tensor(float(thresh), dtype=F32), torch.as_tensor(wmax, dtype=F32).reshape(()))
    keep = (w_sel.to(F32) >= thr) & (hit != 0).unsqueeze(1)
    fine = keep.unsqueeze(2).expand(-1, -1, scale).reshape(N, Sc * scale)
    return torch.nonzero(fine), prefill_ref(N, Sc * scale, sigma_default)


def voxel_select_ref(vox, thresh, o, d, rows, bmin, bmax, sigma_default, hit):
    """ray_bounds_ref.select_rows behind the flag."""
    idx, out_c = B.select_rows(vox, thresh, o, d, rows, bmin, bmax, sigma_default)
    return filter_by_ray(idx, hit), out_c


def oracle_select_on_hits(w_sel, thresh, scale, hit):
    """The oracle's own selection (oracle.select_fine, whose maximum is w_sel's) filtered by ray: what select_fine_ref gives with
    wmax = w_sel.max() whenever no weight is NaN."""
    return filter_by_ray(O.select_fine(w_sel, O.RenderCfg(weight_thresh=float(thresh), scale=int(scale))), hit)
