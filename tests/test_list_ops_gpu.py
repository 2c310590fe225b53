"""The fine pass's (ray, sample) list at the sizes the train step runs it at (csrc/select.hip): the exclusive scan in each of its
regimes, and the random cap where a workgroup's chunk takes several passes, both against exact host references -- everything with
torch.equal.

select_scan_kernel gives every one of its 1024 threads a run of per(N) = ceil(N / 1024) rounded up to a multiple of 4 rays: one int4
per thread up to N = 4096, up to 16 of them up to N = 65536, a scalar loop beyond that or when a workspace is not 16-byte aligned;
the last run of a vector regime is ragged unless N is a multiple of 4.  The scan has no entry point of its own: it is reached through
the selection, whose list (and whose out_f prefill) oracle.mcnerf_oracle.select_fine restates.

cap_random keeps the `keep` smallest keys hash32(seed, position) of the first K' = min(*count, max_rows) rows, in list order
(tests/list_ref.py: cap_random_ref).  Its kernels run min(ceil(max_rows / 256), 2048) workgroups, each over a chunk of
ceil(K' / workgroups) rounded up to a multiple of 256 rows, 256 rows per pass, carrying the write position and the tie count from pass
to pass: CAP_CASES names the chunk of every case."""
import numpy as np
import pytest
import torch

from list_ref import cap_random_ref, scan_ref
from oracle import mcnerf_oracle as O

pytestmark = pytest.mark.gpu
SC, SCALE = 3, 2                 # counts per ray in {0, 2, 4, 6}
SENTINEL = -7


def _ops():
    from mc_nerf_amd import ops
    return ops


def per_of(N):
    """Rays per thread of select_scan_kernel."""
    return (((N + 1023) // 1024) + 3) & ~3


def scan_case(N, L=None):
    """Weights spread around the default threshold (three in four above it), with two stretches of L rows (default: 64 runs and 7
    rows, more than one wave of the scan owns) overwritten: [N/3, N/3 + L) with zeros (count 0: a long run of equal offsets), and the
    L rows behind it with weights above the threshold (count Sc * scale).  -> (w, cfg, the oracle's list, the oracle's counts per
    ray, (zero rows, full rows))"""
    g = torch.Generator().manual_seed(N)
    w = torch.rand(N, SC, generator=g) * 4e-3
    L = 64 * per_of(N) + 7 if L is None else L
    a = N // 3
    assert a + 2 * L <= N
    zero, full = (a, a + L), (a + L, a + 2 * L)
    w[zero[0]:zero[1]] = 0.0
    w[full[0]:full[1]] = 5e-3
    cfg = O.RenderCfg(samples=SC, scale=SCALE)
    ref = O.select_fine(w, cfg)
    counts = torch.bincount(ref[:, 0], minlength=N)
    # the case is what it says: rays without a sample, rays with every sample, every count between, neither everything nor nothing
    assert bool((counts[zero[0]:zero[1]] == 0).all()) and bool((counts[full[0]:full[1]] == SC * SCALE).all())
    assert int(counts.min()) == 0 and int(counts.max()) == SC * SCALE and counts.unique().tolist() == [0, 2, 4, 6]
    assert 0 < ref.shape[0] < N * SC * SCALE
    return w, cfg, ref, counts, (zero, full)


def _wmax(w, dev):
    return w.max().reshape(1).view(torch.int32).to(dev)


def _prefill(cfg, N, S):
    return torch.tensor([cfg.sigma_default, 1.0, 1.0, 1.0]).expand(N, S * cfg.scale, 4)


# 1023 / 1024 / 1025: one int4 per thread, a last run of three / four / one rays and three in four threads idle; 4096: the last size
# with one int4 per thread, every thread busy; 4097 / 4099: two, a last run of one / three rays; 32768: eight; 65535 / 65536: sixteen,
# the last run ragged / whole (the largest vector size); 65537 / 70001: runs of 68 / 72 rays in the scalar loop
SCAN_N = [1023, 1024, 1025, 4096, 4097, 4099, 32768, 65535, 65536, 65537, 70001]


@pytest.mark.parametrize("N", SCAN_N)
def test_scan_regimes_through_select_fine(gpu_device, N):
    ops, dev = _ops(), gpu_device
    w, cfg, ref, _, _ = scan_case(N)
    idx, count, out_f = ops.select_fine(w.to(dev), _wmax(w, dev), cfg.weight_thresh, SCALE, cfg.sigma_default)
    k = int(count.item())
    assert k == ref.shape[0]
    assert torch.equal(idx[:k].cpu().long(), ref)
    assert torch.equal(out_f.cpu(), _prefill(cfg, N, SC))


def _select_raw(w, cfg, dev, rc_off, ro_off):
    """mcnerf_select_fine with ray_counts / ray_offsets as views `off` words into sentinel-filled buffers -> (list, counts, offsets)
    after checking that every word around the views is still the sentinel."""
    from mc_nerf_amd import _lib
    ops = _ops()
    N = w.shape[0]
    bufs = [torch.full((N + 8,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2)]
    rc, ro = bufs[0][rc_off:rc_off + N], bufs[1][ro_off:ro_off + N]
    assert rc.data_ptr() % 16 == 4 * rc_off % 16 and ro.data_ptr() % 16 == 4 * ro_off % 16
    idx = torch.full((N * SC * SCALE, 2), SENTINEL, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("mcnerf_select_fine", w.to(dev), _wmax(w, dev), float(cfg.weight_thresh), N, SC, SCALE, float(cfg.sigma_default),
              rc, ro, idx, count, None, ops._stream())
    k = int(count.item())
    for buf, off in zip(bufs, (rc_off, ro_off)):
        assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + N:] == SENTINEL).all())
    assert bool((idx[k:] == SENTINEL).all())
    return idx[:k].cpu().long(), rc.cpu().long(), ro.cpu().long()


@pytest.mark.parametrize("N, L", [(258, 64), (4097, None)])
def test_scan_at_unaligned_workspaces(gpu_device, N, L):
    """Workspaces 4 bytes past a 16-byte boundary (both, or either one) take the scalar loop: the same list, counts and offsets as
    the aligned call and as the references, and the word in front of each view and the words behind it keep their sentinel -- also in
    the aligned call, whose last int4 store would be the one to overrun."""
    w, cfg, ref, counts, _ = scan_case(N, L=L)
    offsets, total = scan_ref(counts)
    assert total == ref.shape[0]
    for rc_off, ro_off in [(4, 4), (1, 1), (1, 4), (4, 1)]:
        idx, rc, ro = _select_raw(w, cfg, gpu_device, rc_off, ro_off)
        assert torch.equal(idx, ref), (rc_off, ro_off)
        assert torch.equal(rc, counts) and torch.equal(ro, offsets), (rc_off, ro_off)


def _expand(mask, scale):
    """The list of a [N, S] mask: torch.nonzero order, every hit `scale` times."""
    hit = torch.nonzero(mask)
    r = torch.arange(scale)
    return torch.stack([hit[:, :1].expand(-1, scale), hit[:, 1:] * scale + r], -1).reshape(-1, 2)


def test_predicate_edges(gpu_device):
    """N = 5 rays (one ragged workgroup) of Sc = 130 samples (a ragged third wave pass): `>=` at the threshold, the threshold falling
    to the maximum, and the all-zero batch."""
    ops, dev = _ops(), gpu_device
    N, S = 5, 130
    cfg = O.RenderCfg(samples=S, scale=SCALE)
    thr = np.float32(cfg.weight_thresh)                    # the threshold as the kernel receives it
    below, above = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))
    assert below < thr < above

    def run(w):
        idx, count, out_f = ops.select_fine(w.to(dev), _wmax(w, dev), cfg.weight_thresh, SCALE, cfg.sigma_default)
        assert torch.equal(out_f.cpu(), _prefill(cfg, N, S))
        return idx[:int(count.item())].cpu().long()

    # a weight exactly at the threshold is selected, the float below it is not
    w = torch.full((N, S), float(below))
    at, over = [(0, 0), (1, 63), (2, 64), (3, 128), (4, 129)], [(0, 129), (2, 65)]
    for n, j in at:
        w[n, j] = float(thr)
    for n, j in over:
        w[n, j] = float(above)
    mask = torch.zeros(N, S, dtype=torch.bool)
    for n, j in at + over:
        mask[n, j] = True
    want = _expand(mask, SCALE)
    assert want.shape[0] == 7 * SCALE and torch.equal(O.select_fine(w, cfg), want)
    assert torch.equal(run(w), want)

    # wmax < thresh: the threshold is the maximum, and only the entries that hold it are listed
    g = torch.Generator().manual_seed(5)
    w = torch.rand(N, S, generator=g) * 5e-4
    top = [(0, 0), (2, 64), (4, 129)]
    for n, j in top:
        w[n, j] = 6e-4
    mask = torch.zeros(N, S, dtype=torch.bool)
    for n, j in top:
        mask[n, j] = True
    want = _expand(mask, SCALE)
    assert float(w.max()) < thr and torch.equal(O.select_fine(w, cfg), want)
    assert torch.equal(run(w), want)

    # all-zero weights, wmax = 0: every sample is listed
    w = torch.zeros(N, S)
    want = _expand(torch.ones(N, S, dtype=torch.bool), SCALE)
    got = run(w)
    assert got.shape[0] == N * S * SCALE and torch.equal(got, want) and torch.equal(O.select_fine(w, cfg), want)


# ------------------------------------------------------------------------------------------------------------------- the random cap
# (K = *count, max_rows, keep): workgroups x rows per chunk (passes of cap_write_kernel's loop)
CAP_CASES = [
    (50000, 70000, 20000),          # 274 x 256 (1): the size of test_a_ops_gpu.py::test_cap_random_device_side, now exact
    (524288, 524288, 200000),       # 2048 x 256 (1): the last size with one pass per chunk
    (524289, 524289, 200000),       # 2048 x 512 (2): the first with two; 2049 workgroups clamped to 2048
    (600000, 1200000, 1),           # 2048 x 512 (2): one entry kept
    (1100000, 1200000, 400000),     # 2048 x 768 (3)
    (1100000, 1200000, 1099999),    # 2048 x 768 (3): one entry dropped
    (1200000, 1200000, 1199),       # 2048 x 768 (3): one entry in a thousand kept
    (4480000, 4480000, 896000),     # 2048 x 2304 (9): 7000 rays x 640 samples, the 128x5 configuration of the benchmark
    (1300000, 1200000, 400000),     # 2048 x 768 (3): *count beyond max_rows clamps
    (400000, 1200000, 400000),      # 2048 x 256: K = keep, the cap does not bind (the copy path) at a full grid
    (0, 1200000, 400000),           # an empty list
]
CAP_SEEDS = [1234567 * 5 + 11, 0x80000001 - 2**32]       # (the second: the top bit set, as the int32 that holds it)


def _chunk(K, max_rows):
    """(workgroups, rows per chunk) of mcn_launch_cap_random."""
    blocks = min((max_rows + 255) // 256, 2048)
    return blocks, ((min(K, max_rows) + blocks - 1) // blocks + 255) & ~255


@pytest.fixture(scope="module")
def idx_of():
    """(rows, device) -> the list [i // 97, i % 97] on the host and on the device, built once per size."""
    made = {}

    def get(rows, dev):
        if rows not in made:
            i = torch.arange(rows, dtype=torch.int32)
            host = torch.stack([i // 97, i % 97], 1)
            made[rows] = (host, host.to(dev))
        return made[rows]
    return get


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


@pytest.mark.parametrize("seed", CAP_SEEDS)
@pytest.mark.parametrize("K, max_rows, keep", CAP_CASES)
def test_cap_random_equals_the_reference(gpu_device, idx_of, K, max_rows, keep, seed):
    ops, dev = _ops(), gpu_device
    host, idx = idx_of(max_rows, dev)
    want, n = cap_random_ref(host, K, max_rows, keep, seed)
    if min(K, max_rows) > keep:                             # the cap binds: a random subset, not the head of the list
        assert n == keep and not torch.equal(want, host[:keep])
    out = torch.full((keep, 2), SENTINEL, dtype=torch.int32, device=dev)
    idx2, c2 = ops.cap_random(idx, _i32(K, dev), max_rows, keep, _i32(seed, dev), out=out)
    assert idx2 is out and int(c2.item()) == n
    assert torch.equal(idx2[:n].cpu(), want)
    assert bool((idx2[n:] == SENTINEL).all())               # nothing is written beyond the list


def test_cap_random_scratch_and_output_hygiene(gpu_device, idx_of):
    """Whatever the scratch holds on entry -- garbage, or the histograms and per-chunk counts of an earlier call -- the result is
    the same; and with fewer entries than `keep` the rows [K, keep) of the output are not written."""
    from mc_nerf_amd import _lib
    ops, dev = _ops(), gpu_device
    K, max_rows, keep = 1100000, 1200000, 400000
    host, idx = idx_of(max_rows, dev)
    count = _i32(K, dev)
    want = {s: cap_random_ref(host, K, max_rows, keep, s)[0] for s in CAP_SEEDS}
    ws = torch.full((int(_lib.lib().mcnerf_cap_ws_words()),), 0x7FFFFFFF, dtype=torch.int32, device=dev)
    for s in (CAP_SEEDS[0], CAP_SEEDS[1], CAP_SEEDS[0], CAP_SEEDS[0]):      # garbage, then another seed's leavings, then its own
        idx2, c2 = ops.cap_random(idx, count, max_rows, keep, _i32(s, dev), ws=ws)
        assert int(c2.item()) == keep and torch.equal(idx2.cpu(), want[s])
    # a binding call's scratch in front of one that does not bind, and the untouched tail of the output
    for Ks in (1, 255, 257, 1500, keep - 1):
        out = torch.full((keep, 2), SENTINEL, dtype=torch.int32, device=dev)
        idx2, c2 = ops.cap_random(idx, _i32(Ks, dev), max_rows, keep, _i32(CAP_SEEDS[0], dev), ws=ws, out=out)
        assert int(c2.item()) == Ks and torch.equal(idx2[:Ks], idx[:Ks]) and bool((idx2[Ks:] == SENTINEL).all())
    with pytest.raises(_lib.McnerfError, match="cap_random: ws must hold"):
        ops.cap_random(idx, count, max_rows, keep, _i32(1, dev), ws=ws[:-1])
    with pytest.raises(_lib.McnerfError, match="cap_random: out must hold"):
        ops.cap_random(idx, count, max_rows, keep, _i32(1, dev), out=out[:-1])


@pytest.mark.parametrize("keep", [1, 255, 256, 257, 70000])
def test_cap_gather(gpu_device, idx_of, keep):
    """One workgroup's worth of rows less one, exactly, plus one; one row; the whole permutation."""
    ops, dev = _ops(), gpu_device
    K = 70000
    host, idx = idx_of(K, dev)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    idx2, count = ops.cap_gather(idx, perm.to(dev), keep)
    assert int(count.item()) == keep and idx2.shape == (keep, 2)
    assert torch.equal(idx2.cpu(), host[perm[:keep]])
    assert not torch.equal(host[perm[:keep]], host[:keep]) or keep == 1
