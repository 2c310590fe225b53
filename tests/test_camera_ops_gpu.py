"""camera_fwd_kernel / camera_bwd_kernel (csrc/camera.hip), called through ops.camera_fwd / ops.camera_bwd, against the fp64 restatement of
tests/camera_ref.py on the cases of its table (the inputs tests/test_camera_ref_cpu.py runs through the fp32 oracle), under its bars:
K relative 2^-23, Kinv 1e-7 + 1e-6 max |Kinv|, everything else c * 2^-24 * abs_sum elementwise (camera_ref.TOL).  One line per case
with error / bar of every output is printed.

  every case       C = 1, 63, 64, 65, 130 cameras (64 threads per block: one block short, full, one camera over, two blocks and two
                   over) x P = 1, 5 points x (600, 800), (800, 800) x multipliers with and without negative ones; rotation angles from
                   exactly 0 over theta^2 = 0 / denormal in fp32 up to pi and 4.5, cyclically over the cameras and differently in the two
                   pose sets; all six upstreams; the backward run twice gives the same bits;
  upstream matrix  at C = 65: each upstream alone, all, none -- an absent upstream leaves exactly 0.0 in the gradients it alone reaches;
  branch matrix    the forward with the intrinsic branch, the extrinsic branch, both, neither: the bits of the fullest call;
  C = 0            empty outputs, nothing launched.

Measured on MI355X, largest error / bar over all cases and settings: K 0.50, Kinv 0.08, pose 0.28, calib 0.32, pix_intr 0.33,
pix_extr 0.29, d_wpose 0.27, d_wpose_intr 0.33, d_wfx 0.43, d_wfy 0.41 (both with dKinv alone), d_wux 0.27, d_wuy 0.30."""
import pytest
import torch

import camera_ref as R

pytestmark = pytest.mark.gpu

_CACHE = {}


def _ops():
    from mc_nerf_amd import ops
    return ops


def _case(name, dev):
    """(host inputs, device inputs) of a table case: made once, shared, never written to."""
    if name not in _CACHE:
        inp = R.make(name)
        _CACHE[name] = (inp, {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()})
    return _CACHE[name]


def _ref(name, m="all"):
    if ("ref", name, m) not in _CACHE:
        _CACHE["ref", name, m] = R.reference(R.make(name), R.MATRIX[m])
    return _CACHE["ref", name, m]


def _fwd(d, intr=True, extr=True):
    out = _ops().camera_fwd(*(d[k] for k in R.PARAMS), d["H"], d["W"], d["wpts_intr"] if intr else None, d["wpts_extr"] if extr else None)
    torch.cuda.synchronize()
    return dict(zip(R.OUTPUTS, out))


def _bwd(d, ups=R.UPSTREAMS):
    up = {u: (d[u] if u in ups else None) for u in R.UPSTREAMS}
    grads = _ops().camera_bwd(*(d[k] for k in R.PARAMS), d["H"], d["W"], up["dK"], up["dKinv"], up["dpose"], up["dcalib"],
                              wpts_intr=d["wpts_intr"], wpts_extr=d["wpts_extr"], dpix_intr=up["dpix_intr"], dpix_extr=up["dpix_extr"])
    torch.cuda.synchronize()
    return dict(zip(R.GRADS, grads))


def _check(label, got, ref):
    fracs, _, bad = R.compare(label, got, ref)
    print(R.line(label, fracs))
    assert not bad, "\n".join(bad)


def _same_bits(label, got, want):
    for k, a in got.items():
        if a is not None:
            assert torch.equal(a.view(torch.int32), want[k].view(torch.int32)), f"[{label}] {k}: the bits differ"


@pytest.mark.parametrize("name", list(R.CASES))
def test_matches_the_fp64_reference(gpu_device, name):
    _, d = _case(name, gpu_device)
    got = {**_fwd(d), **_bwd(d)}
    assert all(got[k] is not None and got[k].dtype == torch.float32 for k in R.OUTPUTS + R.GRADS)
    _check(name, got, _ref(name))
    _same_bits(name + ", backward repeated", _bwd(d), got)


@pytest.mark.parametrize("m", list(R.MATRIX))
def test_upstream_matrix(gpu_device, m):
    _, d = _case(R.MATRIX_CASE, gpu_device)
    got = _bwd(d, R.MATRIX[m])
    _check(f"{R.MATRIX_CASE}, upstream {m}", got, _ref(R.MATRIX_CASE, m))
    reached = {g for u in R.MATRIX[m] for g in R.REACHES[u]}
    for g in R.GRADS:
        if g not in reached:
            assert int(torch.count_nonzero(got[g])) == 0, f"upstream {m}: {g} is not exactly zero"
        else:
            assert int(torch.count_nonzero(got[g])) == got[g].numel(), f"upstream {m}: {g} has zeros"


@pytest.mark.parametrize("intr", [True, False])
@pytest.mark.parametrize("extr", [True, False])
def test_forward_branches(gpu_device, intr, extr):
    _, d = _case(R.MATRIX_CASE, gpu_device)
    got, full = _fwd(d, intr, extr), _fwd(d)
    assert (got["pix_intr"] is not None) == intr and (got["pix_extr"] is not None) == extr
    assert all(got[k] is not None for k in ("K", "Kinv", "pose", "calib"))
    label = f"{R.MATRIX_CASE}, intrinsic branch {'on' if intr else 'off'}, extrinsic branch {'on' if extr else 'off'}"
    _check(label, got, _ref(R.MATRIX_CASE))
    _same_bits(label + " against the fullest call", got, full)


def test_no_cameras(gpu_device):
    ops, dev = _ops(), gpu_device
    e = lambda *shape: torch.empty(*shape, device=dev)
    par = (e(0, 6), e(0, 6), e(0), e(0), e(0), e(0))
    K, Kinv, pose, calib, pi, pe = ops.camera_fwd(*par, 600, 800, e(0, 5, 3), e(0, 5, 3))
    assert K.shape == Kinv.shape == (0, 3, 3) and pose.shape == calib.shape == (0, 3, 4) and pi.shape == pe.shape == (0, 5, 2)
    grads = ops.camera_bwd(*par, 600, 800, e(0, 3, 3), e(0, 3, 3), e(0, 3, 4), e(0, 3, 4), wpts_intr=e(0, 5, 3), wpts_extr=e(0, 5, 3),
                           dpix_intr=e(0, 5, 2), dpix_extr=e(0, 5, 2))
    assert [tuple(g.shape) for g in grads] == [(0, 6), (0, 6), (0,), (0,), (0,), (0,)]
    torch.cuda.synchronize()
