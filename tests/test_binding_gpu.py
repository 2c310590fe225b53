"""`_lib.call` on device tensors (mc_nerf_amd/_lib.py: the binding derived from include/mcnerf.h): a tensor whose dtype is not the
header's element type, a non-contiguous tensor and a tensor at a host-array position are refused before anything launches, by entry
point and parameter name, and the sentinel-filled outputs keep every value; tensors and their raw addresses give the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = -7


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _untouched(*outs):
    torch.cuda.synchronize()
    return all(bool((o == SENTINEL).all()) for o in outs)


def test_wrong_dtype_at_an_int32_pointer_is_refused(gpu_device):
    from mc_nerf_amd import _lib
    idx64 = torch.zeros(4, 2, dtype=torch.int64, device=gpu_device)
    perm = torch.arange(4, dtype=torch.int64, device=gpu_device)
    idx_out = torch.full((4, 2), SENTINEL, dtype=torch.int32, device=gpu_device)
    count = torch.full((1,), SENTINEL, dtype=torch.int32, device=gpu_device)
    with pytest.raises(_lib.McnerfError, match=r"mcnerf_cap_gather: idx_in .*torch\.int32.*torch\.int64"):
        _lib.call("mcnerf_cap_gather", idx64, perm, 4, idx_out, count, _stream())
    assert _untouched(idx_out, count)


def test_non_contiguous_tensor_is_refused(gpu_device):
    from mc_nerf_amd import _lib
    x = torch.rand(5, 3, device=gpu_device).t()                      # [3,5], strides (1, 3)
    assert tuple(x.shape) == (3, 5) and not x.is_contiguous()
    out = torch.full((3, 27), float(SENTINEL), device=gpu_device)
    with pytest.raises(_lib.McnerfError, match=r"mcnerf_encode: x .*contiguous"):
        _lib.call("mcnerf_encode", x, torch.ones(4, device=gpu_device), 3, 4, out, _stream())
    assert _untouched(out)


def test_float_tensor_at_a_void_pointer_is_refused(gpu_device):
    from mc_nerf_amd import _lib, ops
    net = ops.Net(4, 32, 2)
    params = torch.zeros(ops.param_count(net), device=gpu_device)
    nbytes = [int(_lib.lib().mcnerf_packed_bytes_16(*net.triple, 0, b)) for b in (0, 1)]
    fwd32 = torch.full((nbytes[0] // 4,), float(SENTINEL), device=gpu_device)
    bwd = torch.full((nbytes[1],), 256 + SENTINEL, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(_lib.McnerfError, match=r"mcnerf_pack_weights_16: packed_fwd .*torch\.uint8.*torch\.float32"):
        _lib.call("mcnerf_pack_weights_16", *net.triple, params, fwd32, bwd, 0, None, _stream())
    assert _untouched(fwd32) and bool((bwd == 256 + SENTINEL).all())


def test_device_tensor_at_a_host_array_is_refused(gpu_device):
    from mc_nerf_amd import _lib, ops
    em = ops.ErrorMap(2, 8, 8, 4, gpu_device)
    em.cdf.fill_(SENTINEL)
    n = 6
    u = torch.rand(n, 2, device=gpu_device)
    pix = torch.full((n,), SENTINEL, dtype=torch.int64, device=gpu_device)
    seg_cam = torch.tensor([0, 1], dtype=torch.int32, device=gpu_device)
    _, start, K, _ = ops._seg_arrays([0, 1], [0, 3, 6])
    with pytest.raises(_lib.McnerfError, match=r"mcnerf_errmap_sample: seg_cam .*host array"):
        _lib.call("mcnerf_errmap_sample", em.err, *em.geom, seg_cam, start, K, n, 0.5, u, em.cdf, pix, _stream())
    assert _untouched(pix, em.cdf)


def test_tensors_and_their_addresses_give_the_same_bits(gpu_device):
    from mc_nerf_amd import _lib
    x, w = torch.rand(5, 3, device=gpu_device) * 4.0 - 2.0, torch.rand(4, device=gpu_device)
    a, b = (torch.full((5, 27), float(SENTINEL), device=gpu_device) for _ in range(2))
    _lib.call("mcnerf_encode", x, w, 5, 4, a, _stream())
    _lib.call("mcnerf_encode", x.data_ptr(), w.data_ptr(), 5, 4, b.data_ptr(), _stream())
    assert torch.equal(a, b) and torch.equal(a[:, :3], x) and not bool((a == SENTINEL).any())
