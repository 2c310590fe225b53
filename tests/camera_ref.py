"""fp64 restatement of the camera parametrisation of csrc/camera.hip (camera_fwd_kernel / camera_bwd_kernel): the formulas of
oracle.mcnerf_oracle.se3_to_SE3, intrinsics_from_weights and inverse_intrinsic evaluated in float64 on fp32 inputs, and the ONE table of
cases that tests/test_camera_ref_cpu.py (fp32 oracle against this restatement, no GPU) and tests/test_camera_ops_gpu.py (the kernels
against it) both run.  Not a test module.

    s = |w|^2,  A, B, C = sum_{i<=10} (-1)^i s^i / ((2i+1)!, (2i+2)!, (2i+3)!)      the reference's 11-term series, NOT sin and cos
    [R|t] = [I + A wx + B wx^2 | (I + B wx + C wx^2) u]                              wx the skew matrix of w, (w, u) = a row of wpose
    K = [[|W wfx|, 0, |W/2 wux|], [0, |W wfy|, |H/2 wuy|], [0, 0, 1]],  Kinv its inverse (closed form; test_camera_ref_cpu.py compares it
        with torch.linalg.inv)
    pix = K [R|t] [x, 1],  (pix0 / pix2, pix1 / pix2)                                pix_intr through calib = SE3(wpose_intr), pix_extr through pose
    gradients: fp64 autograd of sum(output * upstream) over the upstreams given

`abs_sum` of an output or a gradient is the SAME computation with every added term replaced by its magnitude: the inputs and
upstreams by their absolute values, every minus sign (series, skew matrix, -ux / fx) by a plus, and d (1 / q) = +1 / q^2 (the
denominators themselves keep their true values).  Everything but the reciprocals is then a polynomial with positive coefficients, and
the autograd gradient of such a polynomial is the sum of the magnitudes of the terms of the true gradient.  An fp32 evaluation is
judged against c * 2^-24 * abs_sum, elementwise: a rotation by 4.5 rad sums series terms of size sinh(4.5) / 4.5 = 10 into an entry of
size 1, and a gradient row is a sum of mixed signs over the points of its camera.

Inputs of a case (`make`), all fp32: rotation vectors = random unit axes times theta, theta assigned to the cameras cyclically from
THETAS (C >= 63; the second pose set shifted by 5 places, so that a camera pairs two different regimes) or drawn from U(0.2, 1.2)
(C = 1); translations U(-1, 1); multipliers 1 +- 0.3 (uniform), in the "neg" cases with one negative multiplier of each kind planted in
four different cameras; P calibration points per camera and pose set, placed 2 .. 6 in front of the camera they are projected by
(x = R^T (y - t) of a point y of the camera frame, formed in fp64 and rounded); upstreams N(0,1), dKinv 100 N(0,1)."""
import itertools
import math

import torch

from oracle import mcnerf_oracle as O

PI32 = float(torch.tensor(math.pi, dtype=torch.float32))
# in fp32 theta^2 is 0 at 1e-30, denormal at 1e-20 and 8 x the smallest normal number at 3e-19 (where the squares of the smaller
# components of w are still denormal)
THETAS = (0.0, 1e-30, 1e-20, 3e-19, 1e-8, 1e-4, 1e-2, 0.5, 1.0, 2.0, 3.1, PI32, 4.5)
SHIFT = 5                       # pose set 2 of camera c has THETAS[(c + SHIFT) % 13]

PARAMS = ("wpose", "wpose_intr", "wfx", "wfy", "wux", "wuy")
OUTPUTS = ("K", "Kinv", "pose", "calib", "pix_intr", "pix_extr")
UPSTREAMS = ("dK", "dKinv", "dpose", "dcalib", "dpix_intr", "dpix_extr")           # UPSTREAMS[i] is the upstream of OUTPUTS[i]
GRADS = tuple("d_" + p for p in PARAMS)
GROUP = {"pose": "se3", "calib": "se3", "pix_intr": "pix", "pix_extr": "pix", "d_wpose": "d_pose", "d_wpose_intr": "d_pose",
         "d_wfx": "d_mult", "d_wfy": "d_mult", "d_wux": "d_mult", "d_wuy": "d_mult"}
# The bars.  K: relative 2^-23 (two roundings: W * w, or W / 2 * w).  Kinv: 1e-7 + 1e-6 max |Kinv| (test_camera_parametrisation_fwd_bwd).
# Every other output: c * 2^-24 * abs_sum elementwise, c = the smallest power of two for which the fp32 oracle with fp32 autograd stays
# within HALF the bar on every case of the table and every setting of MATRIX (c >= 2 x the worst ratio |oracle - fp64| / (2^-24 abs_sum)).
# Worst ratios measured on the CPU by test_camera_ref_cpu.py (never the kernel's):
TOL = {
    "se3": 8.0,         # pose, calib:                  worst ratio 2.55 (C65_P5_600x800_neg)
    "pix": 8.0,         # pix_intr, pix_extr:           worst ratio 2.66 (C63_P1_600x800_neg)
    "d_pose": 16.0,     # d_wpose, d_wpose_intr:        worst ratio 5.22 (C130_P1_800x800_pos)
    "d_mult": 8.0,      # d_wfx, d_wfy, d_wux, d_wuy:   worst ratio 3.82 (C65_P5_600x800_pos, dKinv alone)
}
# (K: the oracle's worst error is 1.00 x 2^-24 |K|, Kinv: 0.10 of its bar)
U24 = 2.0 ** -24


def _case(C, P, H, W, neg, seed):
    return dict(C=C, P=P, H=H, W=W, neg=neg, seed=seed)


CASES = {}
for _i, (_C, _P, (_H, _W), _neg) in enumerate(itertools.product((1, 63, 64, 65, 130), (1, 5), ((600, 800), (800, 800)), (False, True))):
    CASES[f"C{_C}_P{_P}_{_H}x{_W}_{'neg' if _neg else 'pos'}"] = _case(_C, _P, _H, _W, _neg, 100 + _i)
MATRIX_CASE = "C65_P5_600x800_pos"
# the upstream and branch matrix, run on MATRIX_CASE: name -> the upstreams that are given (every other one is null)
MATRIX = {k: (k,) for k in UPSTREAMS}
MATRIX["all"] = UPSTREAMS
MATRIX["none"] = ()
# (dpix_intr alone IS "only dpix_intr, with dcalib null", dpix_extr alone "only dpix_extr")
# which gradients an upstream reaches; an absent upstream leaves exactly 0.0 in the gradients that depend on it alone
REACHES = {"dK": ("d_wfx", "d_wfy", "d_wux", "d_wuy"), "dKinv": ("d_wfx", "d_wfy", "d_wux", "d_wuy"), "dpose": ("d_wpose",),
           "dcalib": ("d_wpose_intr",), "dpix_intr": ("d_wpose_intr", "d_wfx", "d_wfy", "d_wux", "d_wuy"),
           "dpix_extr": ("d_wpose", "d_wfx", "d_wfy", "d_wux", "d_wuy")}


def thetas(C):
    """(theta of wpose, theta of wpose_intr) per camera, python floats; None where the angle is drawn at random (C < 63)."""
    if C < 63:
        return None
    return [THETAS[c % len(THETAS)] for c in range(C)], [THETAS[(c + SHIFT) % len(THETAS)] for c in range(C)]


def neg_cameras(C):
    """The cameras whose wfx, wfy, wux, wuy (in this order) are negative in a "neg" case."""
    return [(3 + 17 * k) % C for k in range(4)]


def make(name):
    """The case's fp32 inputs (host): the six parameter tensors, wpts_intr / wpts_extr [C,P,3], the six upstreams, H, W.  Seeded."""
    c = CASES[name]
    C, P = c["C"], c["P"]
    g = torch.Generator().manual_seed(c["seed"])
    th = thetas(C)
    wu = []
    for k in range(2):
        axis = torch.nn.functional.normalize(torch.randn(C, 3, generator=g), dim=-1)
        ang = torch.tensor(th[k], dtype=torch.float64) if th else (0.2 + torch.rand(C, generator=g)).double()
        wu.append(torch.cat([(axis.double() * ang[:, None]).float(), 2.0 * torch.rand(C, 3, generator=g) - 1.0], dim=-1).contiguous())
    ws = [1.0 + 0.3 * (2.0 * torch.rand(C, generator=g) - 1.0) for _ in range(4)]
    if c["neg"]:
        for k, cam in enumerate(neg_cameras(C)):
            ws[k][cam] = -ws[k][cam]
    inp = dict(zip(PARAMS, wu + ws))
    for key, w in (("wpts_extr", wu[0]), ("wpts_intr", wu[1])):
        Rt = _se3(w.double(), False)
        y = torch.cat([2.0 * torch.rand(C, P, 2, generator=g) - 1.0, 2.0 + 4.0 * torch.rand(C, P, 1, generator=g)], dim=-1).double()
        inp[key] = ((y - Rt[:, None, :, 3]) @ Rt[:, :, :3]).float().contiguous()           # rows: R^T (y - t)
    inp["dK"], inp["dKinv"] = torch.randn(C, 3, 3, generator=g), 100.0 * torch.randn(C, 3, 3, generator=g)
    inp["dpose"], inp["dcalib"] = torch.randn(C, 3, 4, generator=g), torch.randn(C, 3, 4, generator=g)
    inp["dpix_intr"], inp["dpix_extr"] = torch.randn(C, P, 2, generator=g), torch.randn(C, P, 2, generator=g)
    inp["H"], inp["W"] = c["H"], c["W"]
    return inp


class _AbsInv(torch.autograd.Function):
    """1 / q_true whose derivative flows to q_abs with its MAGNITUDE, +1 / q_true^2."""
    @staticmethod
    def forward(ctx, q_abs, q_true):
        ctx.save_for_backward(q_true)
        return 1.0 / q_true

    @staticmethod
    def backward(ctx, g):
        (q,) = ctx.saved_tensors
        return g / (q * q), None


def _series(s, absolute):
    A, B, C = torch.zeros_like(s), torch.zeros_like(s), torch.zeros_like(s)
    dA = dB = dC = 1.0
    pw = torch.ones_like(s)
    for i in range(11):
        if i > 0:
            dA *= (2 * i) * (2 * i + 1)
        dB *= (2 * i + 1) * (2 * i + 2)
        dC *= (2 * i + 2) * (2 * i + 3)
        sg = 1.0 if absolute or i % 2 == 0 else -1.0
        A, B, C = A + sg * pw / dA, B + sg * pw / dB, C + sg * pw / dC
        pw = pw * s
    return A, B, C


def _se3(wu, absolute):
    """[C,6] fp64 -> [C,3,4]; absolute: wu holds magnitudes and every term is added."""
    assert wu.dtype == torch.float64
    w, u = wu[:, :3], wu[:, 3:]
    m = 1.0 if absolute else -1.0
    Z = torch.zeros_like(w[:, 0])
    wx = torch.stack([torch.stack([Z, m * w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], Z, m * w[:, 0]], -1),
                      torch.stack([m * w[:, 1], w[:, 0], Z], -1)], -2)
    A, B, C = (t[:, None, None] for t in _series((w * w).sum(-1), absolute))
    I = torch.eye(3, dtype=torch.float64)
    wx2 = wx @ wx
    return torch.cat([I + A * wx + B * wx2, (I + B * wx + C * wx2) @ u[:, :, None]], dim=-1)


def _project(Rt, f, wpts, absolute, p2_true=None):
    """pix = K [R|t] [x,1] -> ((p0 / p2, p1 / p2) [C,P,2], p2 [C,P]); f = (fx, fy, ux, uy), each [C]."""
    cam = wpts @ Rt[:, :, :3].transpose(1, 2) + Rt[:, None, :, 3]
    fx, fy, ux, uy = (t[:, None] for t in f)
    p0, p1, p2 = fx * cam[..., 0] + ux * cam[..., 2], fy * cam[..., 1] + uy * cam[..., 2], cam[..., 2]
    r = _AbsInv.apply(p2, p2_true.abs()) if absolute else 1.0 / p2
    return torch.stack([p0 * r, p1 * r], dim=-1), p2


def forward(par, wpts_intr, wpts_extr, H, W, absolute=False, p2_true=None):
    """fp64 forward of the six parameter tensors `par` (a dict; leaves for autograd) -> dict of OUTPUTS (pix_* None where the points
    are None) and "p2" = (depth of the intr points, of the extr points).  absolute: the abs_sum pass on magnitudes; p2_true then holds
    the true depths."""
    assert all(par[k].dtype == torch.float64 for k in PARAMS)
    mag = (lambda t: t) if absolute else torch.abs
    fx, fy = mag(float(W) * par["wfx"]), mag(float(W) * par["wfy"])
    ux, uy = mag(float(W) / 2 * par["wux"]), mag(float(H) / 2 * par["wuy"])
    Z, One = torch.zeros_like(fx), torch.ones_like(fx)
    K = torch.stack([fx, Z, ux, Z, fy, uy, Z, Z, One], dim=-1).reshape(-1, 3, 3)
    rx, ry = (_AbsInv.apply(fx, fx.detach()), _AbsInv.apply(fy, fy.detach())) if absolute else (1.0 / fx, 1.0 / fy)
    m = 1.0 if absolute else -1.0
    Kinv = torch.stack([rx, Z, m * ux * rx, Z, ry, m * uy * ry, Z, Z, One], dim=-1).reshape(-1, 3, 3)
    pose, calib = _se3(par["wpose"], absolute), _se3(par["wpose_intr"], absolute)
    out = {"K": K, "Kinv": Kinv, "pose": pose, "calib": calib, "pix_intr": None, "pix_extr": None}
    p2 = [None, None]
    for i, (key, Rt, pts) in enumerate((("pix_intr", calib, wpts_intr), ("pix_extr", pose, wpts_extr))):
        if pts is not None:
            out[key], p2[i] = _project(Rt, (fx, fy, ux, uy), pts.double().abs() if absolute else pts.double(), absolute,
                                       None if p2_true is None else p2_true[i])
    out["p2"] = tuple(p2)
    return out


def _grads(par, out, inp, ups, absolute):
    total = None
    for o, u in zip(OUTPUTS, UPSTREAMS):
        if u in ups and out[o] is not None:
            up = inp[u].to(out[o].dtype)
            term = (out[o] * (up.abs() if absolute else up)).sum()
            total = term if total is None else total + term
    if total is not None:
        total.backward()
    return {"d_" + k: (torch.zeros_like(par[k]) if par[k].grad is None else par[k].grad) for k in PARAMS}


def reference(inp, ups=UPSTREAMS, intr=True, extr=True):
    """Every output of both kernels for the inputs of `make`, fp64, with the upstreams `ups` given and the reprojection branches
    `intr` / `extr` evaluated -> dict of OUTPUTS + GRADS + "p2" + "abs_sum" (a dict of the same keys)."""
    wi, we = (inp["wpts_intr"] if intr else None), (inp["wpts_extr"] if extr else None)
    par = {k: inp[k].double().clone().requires_grad_(True) for k in PARAMS}
    out = forward(par, wi, we, inp["H"], inp["W"])
    res = {k: (None if out[k] is None else out[k].detach()) for k in OUTPUTS}
    res["p2"] = tuple(None if t is None else t.detach() for t in out["p2"])
    res.update(_grads(par, out, inp, ups, False))
    apar = {k: inp[k].double().abs().requires_grad_(True) for k in PARAMS}
    aout = forward(apar, wi, we, inp["H"], inp["W"], absolute=True, p2_true=res["p2"])
    res["abs_sum"] = {k: (None if aout[k] is None else aout[k].detach()) for k in OUTPUTS}
    res["abs_sum"].update(_grads(apar, aout, inp, ups, True))
    return res


def oracle32(inp, ups=UPSTREAMS, intr=True, extr=True):
    """The same outputs from the fp32 oracle (O.se3_to_SE3, O.intrinsics_from_weights, O.inverse_intrinsic, the reference's matmuls for
    the pixels) with fp32 autograd."""
    par = {k: inp[k].clone().requires_grad_(True) for k in PARAMS}
    K = O.intrinsics_from_weights(inp["H"], inp["W"], par["wfx"], par["wfy"], par["wux"], par["wuy"])
    out = {"K": K, "Kinv": O.inverse_intrinsic(K), "pose": O.se3_to_SE3(par["wpose"]), "calib": O.se3_to_SE3(par["wpose_intr"]),
           "pix_intr": None, "pix_extr": None}

    def project(wpts, pose):
        cam = torch.cat([wpts, torch.ones_like(wpts[..., :1])], -1) @ pose.transpose(-2, -1)
        pix = cam @ K.transpose(-2, -1)
        return pix[..., :2] / pix[..., 2:]
    if intr:
        out["pix_intr"] = project(inp["wpts_intr"], out["calib"])
    if extr:
        out["pix_extr"] = project(inp["wpts_extr"], out["pose"])
    res = {k: (None if out[k] is None else out[k].detach()) for k in OUTPUTS}
    res.update(_grads(par, out, inp, ups, False))
    return res


def bar(key, ref, tol_scale=1.0):
    """The elementwise (or scalar) bound on |got - ref[key]| in fp64."""
    r = ref[key].double()
    if key == "K":
        return tol_scale * 2.0 ** -23 * r.abs()
    if key == "Kinv":
        return torch.full_like(r, tol_scale * (1e-7 + 1e-6 * float(r.abs().max()))) if r.numel() else r
    return tol_scale * TOL[GROUP[key]] * U24 * ref["abs_sum"][key]


def compare(label, got, ref, tol_scale=1.0):
    """Every output / gradient present (not None) in `got` against `ref` under the bars * tol_scale -> ({key: worst |err| / bar},
    {group: worst |err| / (2^-24 abs_sum)}, list of failure messages naming the camera of the worst miss)."""
    fracs, ratios, bad = {}, {}, []
    for k in OUTPUTS + GRADS:
        if got.get(k) is None:
            continue
        assert ref[k] is not None and tuple(got[k].shape) == tuple(ref[k].shape), (label, k)
        g = got[k].detach().cpu().double()
        if g.numel() == 0:
            continue
        e = (g - ref[k]).abs()
        e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
        b = bar(k, ref, tol_scale)
        over = torch.where(e <= b, torch.zeros_like(e), e / b.clamp_min(1e-300))        # (a zero bar is met by a zero error alone)
        frac = torch.where(e == 0, torch.zeros_like(e), e / b.clamp_min(1e-300))
        fracs[k] = float(frac.max())
        if k in GROUP:
            a = ref["abs_sum"][k]
            ratios[GROUP[k]] = max(ratios.get(GROUP[k], 0.0), float(torch.where(e == 0, torch.zeros_like(e), e / (U24 * a).clamp_min(1e-300)).max()))
        if float(over.max()) > 0:
            at = tuple(int(i) for i in torch.unravel_index(over.reshape(-1).argmax(), over.shape))
            bad.append(f"[{label}] {k}: error {float(e[at]):.3e} > bar {float(b[at]):.3e} at camera {at[0]}, element {at[1:]}: "
                       f"got {float(g[at]):.9g}, reference {float(ref[k][at]):.9g}")
    return fracs, ratios, bad


def line(label, fracs):
    return f"[camera, {label}] error / bar: " + "  ".join(f"{k} {v:.2f}" for k, v in fracs.items())
