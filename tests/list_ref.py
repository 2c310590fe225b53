"""Host restatements of what builds and caps the fine pass's (ray, sample) list (csrc/select.hip, csrc/mcnerf_hash.h), in numpy and
torch on the CPU: the 32-bit hash, the random cap's kept set and the exclusive scan.  Every one is exact, so the tests that use them
compare with equality.  (The selection itself is oracle.mcnerf_oracle.select_fine.)  tests/test_list_ref_cpu.py holds these to brute
force."""
import numpy as np
import torch

_U = np.uint64
_M = _U(0xFFFFFFFF)


def hash32(seed, i):
    """mcn_hash32(seed, i): uint32 arithmetic held in uint64 (a product of two 32-bit words fits).  `seed` and `i` are integers or
    integer arrays (a seed given as a negative int32 is taken as the same 32 bits); -> uint64 holding values below 2^32.

    For a fixed seed this is a bijection of the 32-bit word i: i * odd + seed is one, and so is every step of the murmur3 finaliser
    (x ^= x >> s, x *= odd).  Distinct list positions therefore never share a key: exactly ONE entry of a list equals the random
    cap's threshold key, and the cap's `ties` word is always 1."""
    x = (np.asarray(i).astype(np.int64) & 0xFFFFFFFF).astype(_U)
    sd = (np.asarray(seed).astype(np.int64) & 0xFFFFFFFF).astype(_U)
    x = (x * _U(0x9E3779B9) + sd) & _M
    x ^= x >> _U(16); x = (x * _U(0x85EBCA6B)) & _M; x ^= x >> _U(13); x = (x * _U(0xC2B2AE35)) & _M; x ^= x >> _U(16)
    return x


def cap_random_ref(idx, K, max_rows, keep, seed):
    """mcnerf_cap_random on the host -> (rows [count,2], count): of the first K' = min(K, max_rows) rows of `idx` everything when
    K' <= keep, else the `keep` rows with the smallest keys hash32(seed, position), in list order."""
    Kc = min(int(K), int(max_rows))
    if Kc <= keep:
        return idx[:Kc], Kc
    keys = hash32(seed, np.arange(Kc))
    kept = np.sort(np.argsort(keys, kind="stable")[:keep])
    return idx[torch.from_numpy(kept)], keep


def scan_ref(counts):
    """Exclusive cumulative sum of `counts` and their total, in int64 -> (offsets [N], total)."""
    c = counts.to(torch.int64)
    inc = torch.cumsum(c, 0)
    return inc - c, int(inc[-1]) if c.numel() else 0
