"""fp64 restatement of the ray preamble with per-camera radial lens distortion (csrc/mcnerf_lens.h, csrc/lens.hip; written from
the model's statement in DESIGN.md 4f), differentiable by autograd: tests/multicam_ref.py's ray formula with the undistortion
inserted between the lift and the rotation.

    cam = Kinv [u + 1/2, v + 1/2, 1]^T;   (x_d, y_d) = cam[0..1];   r_d = |(x_d, y_d)|
    r:  the root of  r (1 + k1 r^2 + k2 r^4) = r_d  nearest r_d          (the two-coefficient radial model, OpenCV's meaning and sign)
    s = r / r_d (1 at r_d = 0);   cam <- (s x_d, s y_d, cam[2]);   q = R^T cam;   d = q / |q|;   o = -R^T t

Three ways to the root:
  dtype = float64, solve = "implicit" (the default): 60 plain Newton steps without autograd, then ONE differentiable Newton step at
      the root with a detached f': its derivative is the implicit-function derivative -(df/dtheta) / f'.
  dtype = float64, solve = "unrolled": 60 plain Newton steps, all carried by autograd.  tests/test_lens_cpu.py checks the two agree.
  dtype = float32: exactly the kernel's eight SAFEGUARDED steps (f' floored at 0.25, r clamped to [0, 2 r_d]) in fp32 on the CPU, the
      operations in the kernel's order.  The margins m_f / m_b of tests/test_lens_gpu.py are measured with it.
Every function also returns the root's f' = 1 + 3 k1 r^2 + 5 k2 r^4 per ray, so that a test can state its condition (min f' >= 0.5).
Segment k of the batch is rays [seg_start[k], seg_start[k+1]) of camera seg_cam[k].  Not a test module."""
import torch

KERNEL_STEPS = 8


def cam_of_ray(seg_cam, seg_start, device="cpu"):
    return torch.cat([torch.full((seg_start[k + 1] - seg_start[k],), int(c), dtype=torch.int64) for k, c in enumerate(seg_cam)]).to(device)


def distort(xy, lens):
    """(x_u, y_u) [..., 2] -> (x_d, y_d): the closed-form forward model."""
    q = (xy * xy).sum(-1, keepdim=True)
    return xy * (1.0 + q * (lens[..., :1] + lens[..., 1:] * q))


def _f(r, rd, k1, k2):
    q = r * r
    return r * (1.0 + q * (k1 + k2 * q)) - rd


def _fprime(r, k1, k2):
    q = r * r
    return 1.0 + q * (3.0 * k1 + 5.0 * k2 * q)


def _newton(rd, k1, k2, steps):
    r = rd
    for _ in range(steps):
        r = r - _f(r, rd, k1, k2) / _fprime(r, k1, k2)
    return r


def solve_radius(rd, k1, k2, solve="implicit"):
    """fp64 root of r D(r) = rd, differentiable in rd, k1, k2."""
    if solve == "unrolled":
        return _newton(rd, k1, k2, 60)
    with torch.no_grad():
        r0 = _newton(rd, k1, k2, 60)
    return r0 - _f(r0, rd, k1, k2) / _fprime(r0, k1, k2).detach()


def kernel_radius(rd, k1, k2):
    """The kernel's iteration, step for step, in the dtype of its arguments (fp32 for the margins)."""
    r = rd
    zero, quarter = torch.zeros_like(rd), torch.full_like(rd, 0.25)
    for _ in range(KERNEL_STEPS):
        q = r * r
        fp = 1.0 + q * (3.0 * k1 + (5.0 * k2) * q)
        f = r * (1.0 + q * (k1 + k2 * q)) - rd
        r = r - f / torch.maximum(fp, quarter)
        r = torch.minimum(torch.maximum(r, zero), 2.0 * rd)
    return r


def undistort(xy, lens, solve="implicit"):
    """(x_d, y_d) [..., 2] -> (x_u, y_u) in fp64: the inverse of `distort`."""
    rd = xy.norm(dim=-1, keepdim=True)
    safe = torch.where(rd > 0, rd, torch.ones_like(rd))
    r = solve_radius(safe, lens[..., :1], lens[..., 1:], solve)
    return xy * torch.where(rd > 0, r / safe, torch.ones_like(rd))


def _pixel(pix, W, dtype):
    return torch.stack([(pix % W).to(dtype) + 0.5, torch.div(pix, W, rounding_mode="floor").to(dtype) + 0.5, torch.ones_like(pix).to(dtype)], -1)


def rays_per_ray(P, K, L, pix, W, dtype=torch.float64, solve="implicit"):
    """Per-ray matrices P [n,3,4], K [n,3,3], L [n,2] -> rays_d, rays_o [n,3], f' [n], r_d [n] in `dtype`."""
    P, K, L = P.to(dtype), K.to(dtype), L.to(dtype)
    p = _pixel(pix, W, dtype)
    if dtype == torch.float32:              # the kernel's order: (u K0 + v K1) + K2 per row
        cam = (p[:, None, 0] * K[:, :, 0] + p[:, None, 1] * K[:, :, 1]) + K[:, :, 2]
    else:
        cam = (K @ p.unsqueeze(-1)).squeeze(-1)
    xd, yd, k1, k2 = cam[:, 0], cam[:, 1], L[:, 0], L[:, 1]
    if dtype == torch.float32:
        rd = torch.sqrt(xd * xd + yd * yd)
        r = kernel_radius(rd, k1, k2)
        s = torch.where(rd > 0, r / torch.where(rd > 0, rd, torch.ones_like(rd)), torch.ones_like(rd))
    else:
        rd = torch.sqrt(xd * xd + yd * yd)
        safe = torch.where(rd > 0, rd, torch.ones_like(rd))
        r = solve_radius(safe, k1, k2, solve)
        s = torch.where(rd > 0, r / safe, torch.ones_like(rd))
    cam = torch.stack([s * xd, s * yd, cam[:, 2]], -1)
    R, t = P[:, :, :3], P[:, :, 3]
    q = (R.transpose(1, 2) @ cam.unsqueeze(-1)).squeeze(-1)
    d = q / q.norm(dim=-1, keepdim=True)
    o = -(R.transpose(1, 2) @ t.unsqueeze(-1)).squeeze(-1)
    return d, o, _fprime(r, k1, k2).detach(), rd.detach()


def rays(pose, kinv, lens, seg_cam, seg_start, pix, W, dtype=torch.float64, solve="implicit"):
    """pose [C,3,4], kinv [C,3,3], lens [C,2], pix [n] int64 -> rays_d, rays_o [n,3], f' [n], r_d [n] (multicam_ref.rays with the lens)."""
    c = cam_of_ray(seg_cam, seg_start, pix.device)
    return rays_per_ray(pose[c], kinv[c], lens[c], pix, W, dtype, solve)


def backward(pose, kinv, lens, seg_cam, seg_start, pix, W, g_d, g_o, solve="implicit"):
    """fp64 gradients for the upstream g_d, g_o [n,3] -> dict: d_pose [C,3,4], d_kinv [C,3,3], d_lens [C,2]; abs_sum: the same shapes,
    the sums of the MAGNITUDES of the per-ray terms (what the rounding of a sum of fp32 terms scales with); terms: the per-ray
    terms themselves ([n,3,4], [n,3,3], [n,2]); fprime [n]."""
    C = pose.shape[0]
    c = cam_of_ray(seg_cam, seg_start, pix.device)
    P = pose.detach().double()[c].clone().requires_grad_(True)
    K = kinv.detach().double()[c].clone().requires_grad_(True)
    L = lens.detach().double()[c].clone().requires_grad_(True)
    d, o, fp, _ = rays_per_ray(P, K, L, pix, W, torch.float64, solve)
    ((d * g_d.double()).sum() + (o * g_o.double()).sum()).backward()
    out = {"abs_sum": {}, "terms": {}, "fprime": fp}
    for name, t, shape in (("d_pose", P.grad, (C, 3, 4)), ("d_kinv", K.grad, (C, 3, 3)), ("d_lens", L.grad, (C, 2))):
        out[name] = torch.zeros(shape, dtype=torch.float64).index_add_(0, c, t)
        out["abs_sum"][name] = torch.zeros(shape, dtype=torch.float64).index_add_(0, c, t.abs())
        out["terms"][name] = t
    return out


def kernel_terms(pose, kinv, lens, seg_cam, seg_start, pix, W, g_d, dtype=torch.float32):
    """The per-ray terms of the kernel's backward, by its own formulas in `dtype` (fp32 for the margins): the implicit derivative at
    the final radius of the eight safeguarded steps, f' floored at 0.25.  -> dict: d_R [n,3,3] (from the direction only), d_kinv
    [n,3,3], d_lens [n,2]."""
    c = cam_of_ray(seg_cam, seg_start, pix.device)
    P, K, L, g = pose.to(dtype)[c], kinv.to(dtype)[c], lens.to(dtype)[c], g_d.to(dtype)
    p = _pixel(pix, W, dtype)
    cam = (p[:, None, 0] * K[:, :, 0] + p[:, None, 1] * K[:, :, 1]) + K[:, :, 2]
    xd, yd, k1, k2 = cam[:, 0], cam[:, 1], L[:, 0], L[:, 1]
    rd = torch.sqrt(xd * xd + yd * yd)
    r = kernel_radius(rd, k1, k2)
    s = torch.where(rd > 0, r / torch.where(rd > 0, rd, torch.ones_like(rd)), torch.ones_like(rd))
    cu = torch.stack([s * xd, s * yd, cam[:, 2]], -1)
    R = P[:, :, :3]
    q = (cu[:, 0, None] * R[:, 0] + cu[:, 1, None] * R[:, 1]) + cu[:, 2, None] * R[:, 2]
    inv = 1.0 / torch.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
    dn = q * inv[:, None]
    dot = (dn[:, 0] * g[:, 0] + dn[:, 1] * g[:, 1]) + dn[:, 2] * g[:, 2]
    gq = (g - dn * dot[:, None]) * inv[:, None]
    gcam = (R[:, :, 0] * gq[:, None, 0] + R[:, :, 1] * gq[:, None, 1]) + R[:, :, 2] * gq[:, None, 2]
    d_R = cu[:, :, None] * gq[:, None, :]
    qq = r * r
    fp = torch.maximum(1.0 + qq * (3.0 * k1 + (5.0 * k2) * qq), torch.full_like(qq, 0.25))
    sf = s / fp
    ds1, ds2, dsx = -(sf * qq), -(sf * (qq * qq)), -(sf * (s * s) * (2.0 * k1 + (4.0 * k2) * qq))
    h = gcam[:, 0] * xd + gcam[:, 1] * yd
    hx = h * dsx
    gd = torch.stack([gcam[:, 0] * s + hx * xd, gcam[:, 1] * s + hx * yd, gcam[:, 2]], -1)
    return {"d_R": d_R, "d_kinv": gd[:, :, None] * p[:, None, :], "d_lens": torch.stack([h * ds1, h * ds2], -1)}


# ------------------------------------------------------------------------------------------------------------------ shared inputs
# The inputs of tests/test_lens_gpu.py, built on the host so that the CPU tests can measure the margins on the very same numbers.
# (H, W, C), the step's cameras, rays.  n = 1000 / 5 / 1: several blocks with block 0 straddling segments; one- and two-ray segments;
# empty segments.  [2, 0, 2]: a camera twice, cameras out of order.
CASES = {"a3": (37, 53, 4, [2, 0, 2], 1000), "a1": (37, 53, 4, [2], 1000), "b3": (20, 30, 3, [2, 0, 2], 5), "b3one": (20, 30, 3, [2, 0, 2], 1),
         "b1": (20, 30, 3, [1], 5)}
# |k1| <= 0.08, |k2| <= 0.01, every sign pattern among the first four rows
LENS_ROWS = [[0.08, -0.01], [-0.08, 0.01], [-0.08, -0.01], [0.05, 0.01]]
MAX_FOV = 60            # degrees: r_d <= tan(30 deg) * sqrt(2) * 1.1 < 1.0 at the image corners with the 3 % perturbation below


def make_case(name):
    """pose [C,3,4], kinv [C,3,3] (every camera its own, narrow enough for r_d <= 1), lens [C,2], uint8 images [C, H W, 4], injected
    pixels (the four image corners first: the largest radii), upstream gradients -- host tensors, deterministic."""
    from mc_nerf_amd import ops, synthetic as S
    H, W, C, cams, n = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 11)
    pose, K, fov = S.ball_cameras(0, H=H, W=W)
    ok = torch.tensor([i for i, f in enumerate(fov) if f <= MAX_FOV])
    sel = ok[torch.randperm(ok.numel(), generator=g)[:C]]
    pose = pose[sel].float().contiguous()
    kinv = torch.linalg.inv(K[sel].double()).float()
    kinv = (kinv * (1.0 + 0.03 * torch.randn(C, 3, 3, generator=g))).contiguous()
    lens = torch.tensor(LENS_ROWS[:C], dtype=torch.float32)
    pix = torch.randint(0, H * W, (n,), generator=g)
    corners = torch.tensor([0, W - 1, (H - 1) * W, H * W - 1])
    pix[:min(4, n)] = corners[:min(4, n)]
    return dict(H=H, W=W, C=C, cams=cams, n=n, seg=ops.ray_segments(n, len(cams)), pose=pose, kinv=kinv, lens=lens, pix=pix,
                images=torch.randint(0, 256, (C, H * W, 4), dtype=torch.uint8, generator=g),
                g_d=torch.randn(n, 3, generator=g), g_o=torch.randn(n, 3, generator=g))


def measure_margins(case):
    """The deviation of the fp32 mode from the fp64 mode on one case's inputs, in units of 2^-24:
    fwd: max |d32 - d64| / max |d64|  (the directions; the origins do not see the lens);
    bwd: per tensor, the per-ray relative error of the fp32 terms weighted by the terms' magnitudes, worst entry and camera --
         sum_i |t32_i - t64_i| / sum_i |t64_i| over the camera's rays -- so that the error a sum inherits from its terms is at most
         that figure times abs_sum (the rounding of the summation itself comes on top: the floor of 16 units)."""
    s = make_case(case)
    a = (s["pose"], s["kinv"], s["lens"], s["cams"], s["seg"], s["pix"], s["W"])
    d64, _, fp, rd = rays(*a)
    d32, _, _, _ = rays(*a, dtype=torch.float32)
    u = 2.0 ** -24
    fwd = float((d32.double() - d64).abs().max() / d64.abs().max()) / u
    ref = backward(*a, s["g_d"], s["g_o"])
    t32 = kernel_terms(*a, s["g_d"])
    c = cam_of_ray(s["cams"], s["seg"])
    worst = {}
    # d_R of the direction: the reference's d_pose terms minus the origin's part, i.e. evaluated with g_o = 0
    ref_dir = backward(*a, s["g_d"], torch.zeros_like(s["g_o"]))
    for name, t64 in (("d_R", ref_dir["terms"]["d_pose"][:, :, :3]), ("d_kinv", ref["terms"]["d_kinv"]), ("d_lens", ref["terms"]["d_lens"])):
        w = 0.0
        for cam in set(s["cams"]):
            m = c == cam
            if int(m.sum()) == 0:
                continue
            err = (t32[name][m].double() - t64[m]).abs().sum(0)
            mean = t64[m].abs().sum(0)
            ok = mean > 0
            if bool(ok.any()):
                w = max(w, float((err[ok] / mean[ok]).max()))
        worst[name] = w / u
    return {"fwd": fwd, "bwd": worst, "min_fprime": float(fp.min()), "max_rd": float(rd.max())}


# ------------------------------------------------------------------------------------------------------------------ recovery without a field
RECOVERY_CASE, RECOVERY_STEPS, RECOVERY_LR = "a1", 300, 1e-2      # chosen on the CPU: the fp64 loop ends with |k1 - k1*| = 4e-8 < 1e-3


def recovery_loop(directions, target, C, steps=RECOVERY_STEPS, lr=RECOVERY_LR, dtype=torch.float64, device="cpu"):
    """Fits lens [C,2] from zero by Adam on the mean squared direction error; `directions(lens)` -> rays_d [n,3] of the fixed pixels,
    pose and K.  -> the fitted lens (detached)."""
    lens = torch.zeros(C, 2, dtype=dtype, device=device, requires_grad=True)
    opt = torch.optim.Adam([lens], lr=lr)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        ((directions(lens) - target) ** 2).mean().backward()
        opt.step()
    return lens.detach()
