"""train_loss_kernel, reproj_loss_fwd/bwd_kernel and scale3_kernel (csrc/camera.hip) against the fp64 restatement of tests/loss_ref.py on the
cases of its table (the inputs tests/test_loss_ref_cpu.py runs through fp32 eager torch), under its bars: values 2e-6 max(1, |ref|),
gradients 2e-6 max |ref| + 1e-12.  One line per case with error / bar is printed.

  train_loss   1 .. 70001 rays: one pass of a block short and over (85, 86), one block and two (341, 342), 21 blocks, the cap of 128
               blocks without and with a second grid-stride round (43690, 43691), 70001; 0, 1, 255, 256, 257, 550 reprojection
               points; normalise x with_fine.  The arrival-counter protocol: out[3] is zero after every call, a second call on the
               same buffer gives the same bits, and so does a call on a buffer that holds the 128 partials of a larger one; the
               test's own workspace has 128 guard words behind out[TRAIN_LOSS_OUT], which stay zero (a launch of more than 128
               blocks would write its partials there);
  reproj_loss  n = 1, 255, 256, 257, 550, 1000 points, the upstream 0.37;
  scale3_      absent operands, unequal lengths, one block and many: every element is the fp32 product (one rounding: torch.equal with
               the CPU's), a canary behind each buffer is untouched.

Measured on MI355X, largest error / bar: train_loss total 0.04, L_intr < 0.001, rgb 0.03, d_pd 0.08, d_c 0.04, d_f 0.04;
reproj_loss value < 0.001, d_pd 0.04."""
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu

_CACHE = {}


def _ops():
    from mc_nerf_amd import ops
    return ops


def _case(name, dev):
    """(fp64 reference, device inputs) of a table case: made once, shared, never written to."""
    if name not in _CACHE:
        inp = R.make(name)
        _CACHE[name] = (R.reference(inp), {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()})
    return _CACHE[name]


GUARD = 128                                 # words behind the workspace that no block may write (a block index past the cap would)


def _train_loss(d, ws=None):
    """mcnerf_train_loss called as ops.train_loss calls it, on the first TRAIN_LOSS_OUT words of `ws` (a fresh zeroed buffer of
    TRAIN_LOSS_OUT + GUARD words when None) -> (ws, d_pd | None, d_c, d_f | None)."""
    from mc_nerf_amd import _lib
    ops = _ops()
    pd, rc, rf = d["pd"], d["rgb_c"], d["rgb_f"]
    if ws is None:
        ws = torch.zeros(ops.TRAIN_LOSS_OUT + GUARD, dtype=torch.float32, device=rc.device)
    d_pd = torch.empty_like(pd) if pd is not None else None
    d_c = torch.empty_like(rc)
    d_f = torch.empty_like(rf) if rf is not None else None
    _lib.call("mcnerf_train_loss", pd, d["pt_gt"], pd.numel() // 2 if pd is not None else 0, R.H, R.W, int(d["normalise"]), rc, rf, d["gt"],
              rc.numel(), ws[:ops.TRAIN_LOSS_OUT], d_pd, d_c, d_f, ops._stream())
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws[ops.TRAIN_LOSS_OUT:])) == 0, "words behind out[TRAIN_LOSS_OUT] were written"
    return ws, d_pd, d_c, d_f


def _as_dict(out3, d_pd, d_c, d_f):
    return {"total": out3[0], "l_intr": out3[1], "rgb": out3[2], "d_pd": d_pd, "d_c": d_c, "d_f": d_f}


def _same_bits(label, got, want):
    for k in R.VALUES + R.GRADS:
        assert (got[k] is None) == (want[k] is None), (label, k)
        if got[k] is not None:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), f"[{label}] {k}: the bits differ"


def _counter(out):
    return int(out.view(torch.int32)[3].item())


@pytest.mark.parametrize("name", list(R.CASES))
def test_train_loss_matches_the_fp64_reference(gpu_device, name):
    ops = _ops()
    ref, d = _case(name, gpu_device)
    out3, d_pd, d_c, d_f = ops.train_loss(d["pd"], d["pt_gt"], R.H, R.W, d["normalise"], d["rgb_c"], d["rgb_f"], d["gt"])
    torch.cuda.synchronize()
    got = _as_dict(out3, d_pd, d_c, d_f)
    assert out3.shape == (3,)
    fracs, bad = R.compare(name, got, ref)
    print(R.line(name, fracs))
    assert not bad, "\n".join(bad)
    # the same call on a workspace of the test's own: the counter is zero again, and a second call on it gives the same bits
    ws, *g1 = _train_loss(d)
    assert ws.numel() - GUARD == ops.TRAIN_LOSS_OUT == 4 + R.LOSS_BLOCKS
    assert _counter(ws) == 0, f"[{name}] out[3] = {_counter(ws)} after the call"
    first = _as_dict(ws[:3].clone(), *g1)
    _same_bits(name + ", own workspace", first, got)
    ws2, *g2 = _train_loss(d, ws=ws)
    assert ws2 is ws and _counter(ws) == 0, f"[{name}] out[3] = {_counter(ws)} after the second call"
    _same_bits(name + ", repeated on the same workspace", _as_dict(ws[:3], *g2), first)


def test_train_loss_without_points(gpu_device):
    ref, d = _case("points_0", gpu_device)
    assert d["pd"] is None and d["pt_gt"] is None
    out3, d_pd, d_c, d_f = _ops().train_loss(None, None, R.H, R.W, True, d["rgb_c"], d["rgb_f"], d["gt"])
    assert d_pd is None and float(out3[1]) == 0.0 and float(out3[0]) == float(out3[2])
    assert ref["d_pd"] is None and float(ref["l_intr"]) == 0.0


def test_stale_partials_do_not_leak(gpu_device):
    """70001 rays fill all 128 partials out[4..]; 86 rays on the SAME workspace then run one block, which must add out[4] alone."""
    _, big = _case("rays_70001", gpu_device)
    _, small = _case("rays_86", gpu_device)
    assert R.blocks_of(70001) == R.LOSS_BLOCKS and R.blocks_of(86) == 1
    ws, *_ = _train_loss(big)
    assert int(torch.count_nonzero(ws[4:])) == R.LOSS_BLOCKS and _counter(ws) == 0             # (the guard words behind them are zero)
    fresh, *gf = _train_loss(small)
    ws, *gs = _train_loss(small, ws=ws)
    assert _counter(ws) == 0
    _same_bits("86 rays after 70001 on the same workspace", _as_dict(ws[:3], *gs), _as_dict(fresh[:3], *gf))
    assert int(torch.count_nonzero(ws[5:])) == R.LOSS_BLOCKS - 1                   # (the stale partials are still there: they were not read)


@pytest.mark.parametrize("n", R.REPROJ_N)
def test_reproj_loss_matches_the_fp64_reference(gpu_device, n):
    ops, dev = _ops(), gpu_device
    inp = R.make_reproj(n)
    ref = R.reproj_reference(inp)
    pd, gt = inp["pd"].to(dev), inp["gt"].to(dev)
    value = ops.reproj_loss_fwd(pd, gt, R.H, R.W)
    d_pd = ops.reproj_loss_bwd(pd, gt, R.H, R.W, torch.tensor(R.DLOSS, device=dev))
    torch.cuda.synchronize()
    assert value.shape == () and d_pd.shape == (n, 2)
    fracs, bad = R.compare(f"reproj_loss n = {n}", {"value": value, "d_pd": d_pd}, ref, values=("value",), grads=("d_pd",))
    print(R.line(f"reproj_loss n = {n}", fracs))
    assert not bad, "\n".join(bad)
    assert torch.equal(ops.reproj_loss_bwd(pd, gt, R.H, R.W, torch.tensor(R.DLOSS, device=dev)), d_pd)
    assert torch.equal(ops.reproj_loss_fwd(pd, gt, R.H, R.W), value)


@pytest.mark.parametrize("lengths", R.SCALE3_CASES, ids=lambda l: "-".join(str(v) for v in l))
def test_scale3(gpu_device, lengths):
    ops, dev = _ops(), gpu_device
    g = torch.Generator().manual_seed(5000 + sum(v or 0 for v in lengths))
    CANARY = 12345.0
    host, bufs, views = [], [], []
    for n in lengths:
        if n is None:
            host.append(None), bufs.append(None), views.append(None)
            continue
        h = torch.randn(n, generator=g)
        b = torch.cat([h, torch.tensor([CANARY])]).to(dev)
        host.append(h), bufs.append(b), views.append(b[:n])
    ops.scale3_(views[0], views[1], views[2], torch.tensor(R.SCALE3_G, device=dev))
    torch.cuda.synchronize()
    s = torch.tensor(R.SCALE3_G, dtype=torch.float32)
    for name, h, b in zip("abc", host, bufs):
        if h is not None:
            assert torch.equal(b[:-1].cpu(), h * s), f"{name}: not the fp32 product"
            assert float(b[-1]) == CANARY, f"{name}: the element behind the buffer was written"
