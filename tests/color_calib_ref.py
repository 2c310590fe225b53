"""fp64 restatement of the colour-calibrated loss of a NeRF-stage train step (written from the contract in
include/mcnerf.h, not from csrc/color_calib.hip), differentiable by autograd:

    g_c = 1 + color_w[c, 0:3],  b_c = color_w[c, 3:6]           camera c observes g_c * rgb + b_c of the rendered colour
    L_rgb  = mean_i,ch (g rgb_c[i] + b - gt[i])^2 + the same for rgb_f      g, b of the camera of ray i's segment
    L_reg  = reg * (1/K) sum_k mean_j color_w[c_k, j]^2                       over the non-empty segments of the step
    L_intr = mean((pd_x - gt_x)^2) / W^2 + mean((pd_y - gt_y)^2) / H^2;  its term is L_intr / (L_intr.detach() + 1e-8) when
             `normalise`, L_intr itself otherwise
    total  = L_intr term + L_rgb + L_reg

Segment k of the batch is rays [seg_start[k], seg_start[k+1]) of camera seg_cam[k].  `grads` also returns, per output, `abs_sum` =
the sum of the MAGNITUDES of the terms that were added into it: a row of d_color is a sum of mixed signs over the rays of its
camera, so an fp32 sum of it is judged against that, not against the (possibly cancelled) result.  Not a test module."""
import torch


def cam_of_ray(seg_cam, seg_start, device="cpu"):
    return torch.cat([torch.full((seg_start[k + 1] - seg_start[k],), int(c), dtype=torch.int64) for k, c in enumerate(seg_cam)]).to(device)


def loss(pd, pt_gt, H, W, normalise, rgb_c, rgb_f, gt, color_w, seg_cam, seg_start, reg):
    """-> dict(total, l_intr, l_rgb, l_reg) of fp64 scalars (pd may be None: no reprojection term)."""
    d = lambda t: None if t is None else t.double()
    pd, pt_gt, rgb_c, rgb_f, gt, color_w = d(pd), d(pt_gt), d(rgb_c), d(rgb_f), d(gt), d(color_w)
    K = len(seg_cam)
    w = color_w[cam_of_ray(seg_cam, seg_start, color_w.device)]
    g, b = 1.0 + w[:, :3], w[:, 3:]
    l_rgb = ((g * rgb_c + b - gt) ** 2).mean()
    if rgb_f is not None:
        l_rgb = l_rgb + ((g * rgb_f + b - gt) ** 2).mean()
    l_reg = torch.zeros((), dtype=torch.float64, device=color_w.device)
    for k, c in enumerate(seg_cam):
        if seg_start[k + 1] > seg_start[k]:
            l_reg = l_reg + (color_w[int(c)] ** 2).mean()
    l_reg = reg * l_reg / K
    l_intr = torch.zeros((), dtype=torch.float64, device=color_w.device)
    term = l_intr
    if pd is not None and pd.numel():
        e = pd.reshape(-1, 2) - pt_gt.reshape(-1, 2)
        l_intr = (e[:, 0] ** 2).mean() / float(W) ** 2 + (e[:, 1] ** 2).mean() / float(H) ** 2
        term = l_intr / (l_intr.detach() + 1e-8) if normalise else l_intr
    return {"total": term + l_rgb + l_reg, "l_intr": l_intr, "l_rgb": l_rgb, "l_reg": l_reg}


def grads(pd, pt_gt, H, W, normalise, rgb_c, rgb_f, gt, color_w, seg_cam, seg_start, reg, upstream=1.0):
    """Value and the autograd gradients of `upstream * total`, fp64: dict(value, l_intr, l_rgb, l_reg, d_pd, d_c, d_f, d_color,
    abs_sum = dict(value, d_pd, d_c, d_f, d_color))."""
    leaf = lambda t: None if t is None else t.detach().double().clone().requires_grad_(True)
    pd_, c_, f_, w_ = leaf(pd), leaf(rgb_c), leaf(rgb_f), leaf(color_w)
    parts = loss(pd_, pt_gt, H, W, normalise, c_, f_, gt, w_, seg_cam, seg_start, reg)
    (upstream * parts["total"]).backward()
    out = {"value": parts["total"].detach(), "l_intr": parts["l_intr"].detach(), "l_rgb": parts["l_rgb"].detach(), "l_reg": parts["l_reg"].detach(),
           "d_pd": None if pd_ is None else pd_.grad, "d_c": c_.grad, "d_f": None if f_ is None else f_.grad, "d_color": w_.grad}
    # the magnitudes added into every entry of d_color: per ray |gr e rgb| (gain) and |gr e| (bias) of both renders, per non-empty
    # segment |2 reg / (6 K) w|; every other output is a single term (or a sum of squares): its own magnitude
    cw, gtd = color_w.detach().double(), gt.detach().double()
    n, K, C = gtd.shape[0], len(seg_cam), cw.shape[0]
    cam = cam_of_ray(seg_cam, seg_start, cw.device)
    g, b = 1.0 + cw[cam, :3], cw[cam, 3:]
    mag = torch.zeros(C, 6, dtype=torch.float64, device=cw.device)
    for rgb in (rgb_c, rgb_f):
        if rgb is None:
            continue
        rgb = rgb.detach().double()
        ge = (2.0 / (3 * n)) * (g * rgb + b - gtd)
        mag.index_add_(0, cam, torch.cat([(ge * rgb).abs(), ge.abs()], 1))
    for k, c in enumerate(seg_cam):
        if seg_start[k + 1] > seg_start[k]:
            mag[int(c)] += (2.0 * reg / (6 * K)) * cw[int(c)].abs()
    absd = lambda t: None if t is None else t.abs()
    out["abs_sum"] = {"value": out["value"].abs(), "d_pd": absd(out["d_pd"]), "d_c": absd(out["d_c"]), "d_f": absd(out["d_f"]),
                      "d_color": abs(upstream) * mag}
    return out
