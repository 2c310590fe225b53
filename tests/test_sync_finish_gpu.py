"""sync_finish_kernel (csrc/optim.hip), the finish of FlatGradSync's one all-reduce, called through ops.sync_finish in ONE process on
hand-built arenas [n_grad summed gradients | n_flags summed "produced a gradient" flags]:

    arena[:n_grad] /= world;   asym += 1 when some flag sum differs from world * local_flags -- once per call, not once per flag.

  n_grad   0, 1, 255, 256, 257 (either side of a 256-thread block), 100003;  n_flags 0, 1, 52, 300 (the flags are compared by block 0
           alone, in a loop of stride 256: 300 takes a second round);  world 1, 2, 3, 8;  gradients N(0,1) * 10^U(-20, 20).
  The quotient is torch's CPU fp32 arena / world bit for bit (the division is IEEE, the build has no fast-math); the flag words are
  untouched; agreeing flags leave asym alone; ONE disagreeing flag -- index 0, 255, 256 -- or three at once raise it by exactly 1, and
  an agreeing call after that leaves it where it was."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_GRAD = (0, 1, 255, 256, 257, 100003)
N_FLAGS = (0, 1, 52, 300)
WORLDS = (1, 2, 3, 8)
ASYM0 = 7                                    # the counter's value before the call


def _ops():
    from mc_nerf_amd import ops
    return ops


def _arena(n_grad, n_flags, world, seed):
    """(host arena with agreeing flags, host local flags)."""
    g = torch.Generator().manual_seed(seed)
    grads = torch.randn(n_grad, generator=g) * 10.0 ** (40.0 * torch.rand(n_grad, generator=g) - 20.0)
    local = (torch.rand(n_flags, generator=g) < 0.5).float()
    return torch.cat([grads, local * float(world)]).contiguous(), local


def _run(arena, n_grad, world, local, asym):
    _ops().sync_finish(arena, n_grad, world, local, asym)
    torch.cuda.synchronize()


def _check_arena(arena, host, n_grad, world):
    want = host[:n_grad] / torch.tensor(float(world), dtype=torch.float32)
    assert torch.equal(arena[:n_grad].cpu().view(torch.int32), want.view(torch.int32)), "arena[:n_grad] is not the fp32 quotient bit for bit"
    assert torch.equal(arena[n_grad:].cpu().view(torch.int32), host[n_grad:].view(torch.int32)), "the flag words were written"


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("n_flags", N_FLAGS)
@pytest.mark.parametrize("n_grad", N_GRAD)
def test_divides_and_leaves_agreeing_flags_alone(gpu_device, n_grad, n_flags, world):
    dev = gpu_device
    host, local = _arena(n_grad, n_flags, world, 1000 * world + 10 * n_flags + n_grad)
    if n_grad:
        mag = host[:n_grad].abs()
        assert n_grad < 255 or (float(mag.min()) < 1e-10 and float(mag.max()) > 1e10)          # the magnitudes span the fp32 range
    arena, asym = host.to(dev), torch.tensor([ASYM0], dtype=torch.int32, device=dev)
    _run(arena, n_grad, world, local.to(dev), asym)
    _check_arena(arena, host, n_grad, world)
    assert int(asym.item()) == ASYM0


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n_grad", [0, 257])
@pytest.mark.parametrize("n_flags,wrong", [(1, (0,)), (52, (0,)), (52, (51,)), (300, (0,)), (300, (255,)), (300, (256,)), (300, (299,)),
                                          (300, (3, 255, 256))])
def test_disagreeing_flags_count_once_per_call(gpu_device, n_grad, n_flags, wrong, world):
    dev = gpu_device
    host, local = _arena(n_grad, n_flags, world, 77 + n_flags + n_grad + world)
    for k in wrong:                                          # another rank produced a gradient where this one did not, or the reverse
        host[n_grad + k] += 1.0 if local[k] == 0 else -1.0
    arena, asym, local_d = host.to(dev), torch.tensor([ASYM0], dtype=torch.int32, device=dev), local.to(dev)
    _run(arena, n_grad, world, local_d, asym)
    _check_arena(arena, host, n_grad, world)
    assert int(asym.item()) == ASYM0 + 1, f"asym rose by {int(asym.item()) - ASYM0} with the flags {wrong} disagreeing"
    # an agreeing call afterwards leaves it where it was
    host2, _ = _arena(n_grad, n_flags, world, 77 + n_flags + n_grad + world)
    arena2 = host2.to(dev)
    _run(arena2, n_grad, world, local_d, asym)
    _check_arena(arena2, host2, n_grad, world)
    assert int(asym.item()) == ASYM0 + 1
