"""tests/list_ref.py, the host restatements that tests/test_list_ops_gpu.py holds the list kernels to, held to brute force themselves:
the hash against a scalar restatement in Python integers, its injectivity, the cap's kept set against Python's `sorted` on (key,
position) tuples and at its edges, the scan against a loop."""
import numpy as np
import pytest
import torch

from list_ref import cap_random_ref, hash32, scan_ref
from test_list_ops_gpu import CAP_CASES, SCAN_N, _chunk, per_of, scan_case

SEEDS = [0, 42, 1234567 * 3 + 11, 0x80000001, 0xFFFFFFFF]


def _hash_int(seed, i):
    """mcn_hash32 in Python integers, one word at a time."""
    x = (i * 0x9E3779B9 + seed) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _idx(n):
    i = torch.arange(n, dtype=torch.int32)
    return torch.stack([i // 97, i % 97], 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_hash32_is_the_scalar_hash(seed):
    i = np.concatenate([np.arange(300), np.array([2**20 - 1, 2**31 - 1, 2**31, 2**32 - 1])])
    assert hash32(seed, i).tolist() == [_hash_int(seed, int(v)) for v in i]
    assert int(hash32(seed, 7)) == _hash_int(seed, 7) and hash32(seed, i).dtype == np.uint64
    if seed >= 2**31:                       # the same 32 bits as an int32, the way a seed tensor holds them
        assert np.array_equal(hash32(seed - 2**32, i), hash32(seed, i))


@pytest.mark.parametrize("seed", SEEDS)
def test_hash32_is_injective(seed):
    """For a fixed seed the hash is a bijection of the 32-bit word i (an odd multiplier plus a constant, then the murmur3 finaliser,
    whose steps are all invertible), so no two list positions share a key: exactly one entry equals the cap's threshold key, its
    `ties` word is 1, and there is no tie case to test."""
    keys = hash32(seed, np.arange(2**20))
    assert int(keys.max()) < 2**32 and np.unique(keys).size == 2**20


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K, keep", [(2, 1), (300, 1), (300, 150), (300, 299), (2000, 777)])
def test_cap_random_ref_is_sorted_tuples(K, keep, seed):
    idx = _idx(K + 5)
    by_key = sorted((_hash_int(seed, i), i) for i in range(K))
    kept = sorted(i for _, i in by_key[:keep])
    rows, count = cap_random_ref(idx, K, K + 5, keep, seed)
    assert count == keep and torch.equal(rows, idx[kept])
    assert kept != list(range(keep)) or keep == 1           # (a random subset, not the head of the list; hash32(0, 0) is 0)


def test_cap_random_ref_edges():
    idx, seed = _idx(1000), 42
    for K, keep in [(0, 10), (1, 1), (10, 10), (9, 10), (700, 1000)]:       # K <= keep: the list as it stands
        rows, count = cap_random_ref(idx, K, 1000, keep, seed)
        assert count == K and torch.equal(rows, idx[:K])
    keys = [_hash_int(seed, i) for i in range(501)]
    rows, count = cap_random_ref(idx, 501, 1000, 500, seed)                 # K = keep + 1: the largest key goes
    drop = keys.index(max(keys))
    assert count == 500 and torch.equal(rows, idx[[i for i in range(501) if i != drop]])
    rows, count = cap_random_ref(idx, 501, 1000, 1, seed)                   # keep = 1: the smallest key stays
    assert count == 1 and torch.equal(rows, idx[[keys.index(min(keys))]])
    a = cap_random_ref(idx, 5000, 600, 200, seed)                           # K > max_rows: max_rows rows count
    b = cap_random_ref(idx, 600, 600, 200, seed)
    assert a[1] == b[1] == 200 and torch.equal(a[0], b[0]) and int((a[0][:, 0] * 97 + a[0][:, 1]).max()) < 600
    rows, count = cap_random_ref(idx, 5000, 600, 600, seed)                 # ... and the cap stops binding at K' = keep
    assert count == 600 and torch.equal(rows, idx[:600])
    assert not torch.equal(cap_random_ref(idx, 600, 600, 200, 43)[0], b[0])  # the seed decides


def test_scan_ref():
    g = torch.Generator().manual_seed(0)
    c = torch.randint(0, 7, (1000,), generator=g, dtype=torch.int32)
    off, total = scan_ref(c)
    run, want = 0, []
    for v in c.tolist():
        want.append(run)
        run += v
    assert off.dtype == torch.int64 and off.tolist() == want and total == run
    big = torch.full((3,), 2**30, dtype=torch.int32)                        # int64: no wrap
    assert scan_ref(big)[0].tolist() == [0, 2**30, 2**31] and scan_ref(big)[1] == 3 * 2**30
    assert scan_ref(torch.zeros(0, dtype=torch.int32))[1] == 0


def test_gpu_cases_reach_what_they_name():
    """tests/test_list_ops_gpu.py: the runs per thread of its scan sizes and the chunks of its cap cases, by the formulas of
    csrc/select.hip -- every regime of the scan (runs of 4, of 8 to 64, beyond 64) and chunks of one, two, three and nine passes."""
    assert [per_of(N) for N in SCAN_N] == [4, 4, 4, 4, 8, 8, 32, 64, 64, 68, 72]
    assert [_chunk(K, m) for K, m, _ in CAP_CASES] == [(274, 256), (2048, 256), (2048, 512), (2048, 512), (2048, 768), (2048, 768),
                                                        (2048, 768), (2048, 2304), (2048, 768), (2048, 256), (2048, 0)]


@pytest.mark.parametrize("N, L", [(N, None) for N in SCAN_N] + [(258, 64)])
def test_gpu_scan_cases_are_not_vacuous(N, L):
    """Each scan case holds (and asserts on the oracle's list) a stretch of rays without a sample and one of rays with every sample,
    each of them longer than the 64 runs one wave of the scan owns."""
    _, _, ref, counts, (zero, full) = scan_case(N, L=L)
    assert scan_ref(counts)[1] == ref.shape[0]
    need = 64 * per_of(N) + 7 if L is None else L
    assert zero == (N // 3, N // 3 + need) and full == (zero[1], zero[1] + need) and full[1] <= N
