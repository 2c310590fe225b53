"""fp64 restatement of the loss kernels of csrc/camera.hip (reproj_loss_fwd/bwd_kernel, train_loss_kernel) and the ONE table of cases that
tests/test_loss_ref_cpu.py (fp32 eager torch against this restatement, no GPU) and tests/test_loss_ops_gpu.py (the kernels against it)
both run.  Not a test module.

    reproj_loss = mean((pd_x - gt_x)^2) / W^2 + mean((pd_y - gt_y)^2) / H^2          over the n points [n,2]
    train_loss:   L_intr = reproj_loss(pd, pt_gt) (0 without points),  rgb = mean((rgb_c - gt)^2) + mean((rgb_f - gt)^2) (rgb_f may be absent)
                  total  = L_intr / (L_intr.detach() + 1e-8) when normalised, L_intr otherwise, + rgb
                  d_pd, d_c, d_f = d total / d (pd, rgb_c, rgb_f)                     fp64 autograd

Inputs (`make`, `make_reproj`), all fp32: target pixels U(0,1) (W, H), predicted pixels = targets + 20 N(0,1); colours and their targets
U(0,1).  (H, W) = (600, 800): the two axes weigh differently.

The ray counts sit on the launch geometry of train_loss_kernel (256 threads, one block per 1024 floats, at most 128 blocks): 3 * 85 = 255
and 3 * 86 = 258 floats around one pass of a block; 341 / 342 rays = 1023 / 1026 floats, one block / two; 43690 / 43691 rays = 131070 /
131073 floats either side of 128 * 1024, where the block count is capped and the grid-stride loop starts; 70001 rays well past it.
The point counts 255, 256, 257 and 550 sit around the 256-thread stride of the last block's reprojection loop."""
import torch
import torch.nn.functional as F

H, W = 600, 800
N_RAYS = (1, 85, 86, 341, 342, 7001, 43690, 43691, 70001)
N_POINTS = (0, 1, 255, 256, 257, 550)
LOSS_BLOCKS, LOSS_THREADS = 128, 256                    # MCN_LOSS_BLOCKS and the block size of train_loss_kernel
# The bars, against fp64: today's bars of test_fused_train_loss_matches_eager_formulation.  Worst |fp32 eager torch - fp64| / bar
# measured on the CPU by test_loss_ref_cpu.py over all cases (it asserts <= 0.5):
TOL = {
    "value": 2e-6,          # total, L_intr, rgb: 2e-6 max(1, |ref|);       worst 0.033 (total, flags_43691_norm1_fine0); reproj_loss < 0.001
    "grad": 2e-6,           # d_pd, d_c, d_f:     2e-6 max |ref| + 1e-12;   worst 0.38 (d_pd, rays_43690; d_c, d_f: 0.04); reproj_loss 0.39 (n = 1)
}
VALUES, GRADS = ("total", "l_intr", "rgb"), ("d_pd", "d_c", "d_f")


def _case(n, np_, normalise, with_fine, seed):
    return dict(n=n, np=np_, normalise=normalise, with_fine=with_fine, seed=seed)


CASES = {}
for _n in N_RAYS:
    CASES[f"rays_{_n}"] = _case(_n, 550, True, True, 1000 + _n)
_seed = 2000
for _n in (86, 7001, 43691):
    for _norm in (True, False):
        for _fine in (True, False):
            CASES[f"flags_{_n}_norm{int(_norm)}_fine{int(_fine)}"] = _case(_n, 550, _norm, _fine, _seed)        # one seed per cell
            _seed += 1
for _np in N_POINTS:
    CASES[f"points_{_np}"] = _case(342, _np, True, True, 3000 + _np)

REPROJ_N = (1, 255, 256, 257, 550, 1000)
DLOSS = 0.37
# scale3_ (a, b, c *= g in place): the lengths (na, nb, nc), None = the operand is absent; g = 0.37
SCALE3_G = 0.37
SCALE3_CASES = ((None, 5, None), (300, 5, 0), (5, 300, 257), (256, 256, 256), (1100, 21003, 21003))


def blocks_of(n):
    """Blocks train_loss_kernel is launched with for n rays."""
    return max(1, min(LOSS_BLOCKS, (3 * n + 1023) // 1024))


def _points(np_, g):
    gt = torch.rand(np_, 2, generator=g) * torch.tensor([float(W), float(H)])
    return (gt + 20.0 * torch.randn(np_, 2, generator=g)).contiguous(), gt.contiguous()


def make(name):
    """The case's fp32 inputs (host): pd, pt_gt [np,2] (None when np = 0), rgb_c, rgb_f (None without the fine render), gt [n,3]."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    pd, pt_gt = _points(c["np"], g) if c["np"] else (None, None)
    rgb_c, rgb_f, gt = (torch.rand(c["n"], 3, generator=g) for _ in range(3))
    return dict(pd=pd, pt_gt=pt_gt, rgb_c=rgb_c, rgb_f=rgb_f if c["with_fine"] else None, gt=gt, normalise=c["normalise"])


def make_reproj(n):
    g = torch.Generator().manual_seed(4000 + n)
    pd, gt = _points(n, g)
    return dict(pd=pd, gt=gt)


def reproj_loss(pd, gt):
    """In the dtype of pd (fp64 for the restatement, fp32 for the eager comparison)."""
    e = pd - gt.to(pd.dtype)
    return (e[:, 0] ** 2).mean() / float(W) ** 2 + (e[:, 1] ** 2).mean() / float(H) ** 2


def reproj_reference(inp, dloss=DLOSS):
    """-> dict(value, d_pd) fp64: the loss and d (dloss * loss) / d pd."""
    pd = inp["pd"].double().clone().requires_grad_(True)
    value = reproj_loss(pd, inp["gt"])
    (dloss * value).backward()
    return {"value": value.detach(), "d_pd": pd.grad}


def reproj_eager32(inp, dloss=DLOSS):
    """The same from fp32 eager torch in the reference's formulation (model/loss.py:45-58)."""
    pd, gt = inp["pd"].clone().requires_grad_(True), inp["gt"]
    value = F.mse_loss(pd[:, 0] / W, gt[:, 0] / W) + F.mse_loss(pd[:, 1] / H, gt[:, 1] / H)
    (dloss * value).backward()
    return {"value": value.detach(), "d_pd": pd.grad}


def reference(inp):
    """-> dict(total, l_intr, rgb, d_pd | None, d_c, d_f | None), fp64."""
    leaf = lambda t: None if t is None else t.double().clone().requires_grad_(True)
    pd, rc, rf = leaf(inp["pd"]), leaf(inp["rgb_c"]), leaf(inp["rgb_f"])
    gt = inp["gt"].double()
    l_intr = torch.zeros((), dtype=torch.float64)
    term = l_intr
    if pd is not None:
        l_intr = reproj_loss(pd, inp["pt_gt"])
        term = l_intr / (l_intr.detach() + 1e-8) if inp["normalise"] else l_intr
    rgb = ((rc - gt) ** 2).mean()
    if rf is not None:
        rgb = rgb + ((rf - gt) ** 2).mean()
    total = term + rgb
    total.backward()
    return {"total": total.detach(), "l_intr": l_intr.detach(), "rgb": rgb.detach(), "d_pd": None if pd is None else pd.grad, "d_c": rc.grad,
            "d_f": None if rf is None else rf.grad}


def eager32(inp):
    """The same from fp32 eager torch, the formulation of test_a_ops_gpu.py::test_fused_train_loss_matches_eager_formulation."""
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    pd, rc, rf = leaf(inp["pd"]), leaf(inp["rgb_c"]), leaf(inp["rgb_f"])
    gt, ptg = inp["gt"], inp["pt_gt"]
    l_intr = torch.zeros(())
    term = l_intr
    if pd is not None:
        l_intr = F.mse_loss(pd[:, 0] / W, ptg[:, 0] / W) + F.mse_loss(pd[:, 1] / H, ptg[:, 1] / H)
        term = l_intr / (l_intr.detach() + 1e-8) if inp["normalise"] else l_intr
    rgb = F.mse_loss(rc, gt) + (F.mse_loss(rf, gt) if rf is not None else 0.0)
    total = term + rgb
    total.backward()
    return {"total": total.detach(), "l_intr": l_intr.detach(), "rgb": rgb.detach(), "d_pd": None if pd is None else pd.grad, "d_c": rc.grad,
            "d_f": None if rf is None else rf.grad}


def compare(label, got, ref, tol_scale=1.0, values=VALUES, grads=GRADS):
    """`got` against `ref` under the bars * tol_scale -> ({key: error / bar}, list of failure messages).  A gradient that the
    reference does not have (None) must be None in `got` too."""
    fracs, bad = {}, []
    for k in values:
        e, b = abs(float(got[k]) - float(ref[k])), tol_scale * TOL["value"] * max(1.0, abs(float(ref[k])))
        fracs[k] = e / b
        if not e <= b:
            bad.append(f"[{label}] {k}: error {e:.3e} > {b:.3e}: got {float(got[k]):.9g}, reference {float(ref[k]):.9g}")
    for k in grads:
        if ref[k] is None:
            assert got[k] is None, (label, k)
            continue
        assert got[k] is not None and tuple(got[k].shape) == tuple(ref[k].shape), (label, k)
        e = (got[k].detach().cpu().double() - ref[k]).abs()
        e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
        b = tol_scale * (TOL["grad"] * float(ref[k].abs().max()) + 1e-12)
        i = int(e.reshape(-1).argmax())
        fracs[k] = float(e.reshape(-1)[i]) / b
        if not float(e.reshape(-1)[i]) <= b:
            bad.append(f"[{label}] {k}: max error {float(e.reshape(-1)[i]):.3e} > {b:.3e} at element {i}: got "
                       f"{float(got[k].reshape(-1)[i]):.9g}, reference {float(ref[k].reshape(-1)[i]):.9g}")
    return fracs, bad


def line(label, fracs):
    return f"[loss, {label}] error / bar: " + "  ".join(f"{k} {v:.3f}" for k, v in fracs.items())
