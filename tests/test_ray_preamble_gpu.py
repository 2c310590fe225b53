"""The six kernels of the ray preamble (csrc/rays.hip: sample_perm, raygen_fwd, raygen_bwd, gather_gt, ray_batch_fwd, ray_batch_bwd)
against tests/golden/ray_preamble.npz, bit for bit.

The fixture was recorded on an MI355X from the library of the commit before the per-ray arithmetic moved into csrc/mcnerf_rays.h
(tests/golden/make_ray_preamble.py, which also holds the cases: they exist once); the single- and the multi-camera kernels had their
own copy of it then.  Equality with that recording is what says that sharing the functions changed no bit.  No tolerance anywhere
except where the order of float atomics is not fixed (below).  The integer path is pinned by arithmetic as well: a uint32 restatement
of the Feistel walk in numpy.  The two lens kernels (csrc/lens.hip) are held the same way to tests/golden/ray_preamble_lens.npz (at the
end of the file)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from list_ref import hash32

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_ray_preamble", os.path.join(GOLDEN, "make_ray_preamble.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)


@pytest.fixture(scope="module")
def recorded():
    return load_golden("ray_preamble")


@pytest.fixture(scope="module")
def got(recorded, gpu_device):
    """Every case, run once."""
    return cases.run(recorded, gpu_device)


def _same(got, recorded, prefix, n_expected):
    keys = sorted(k for k in recorded if k.startswith(prefix))
    assert len(keys) == n_expected, keys
    for k in keys:
        assert got[k].shape == recorded[k].shape and got[k].dtype.kind == recorded[k].dtype.kind, k
        assert np.array_equal(got[k], recorded[k]), (k, int((got[k] != recorded[k]).sum()), "entries differ")


def feistel_perm(i, n, seed):
    """mcn_feistel_perm(i, n, &seed, 0) in numpy: uint32 arithmetic held in uint64 (a product of two 32-bit words fits)."""
    u = np.uint64
    bits = 1
    while bits < 32 and (1 << bits) < n:
        bits += 1
    half = u((bits + 1) // 2)
    mask = u((1 << int(half)) - 1)
    x = np.asarray(i, dtype=u)
    walking = np.ones(x.shape, dtype=bool)
    while walking.any():
        L, R = x >> half, x & mask
        for r in range(6):
            L, R = R, L ^ (hash32((seed + 0x632BE5AB * (r + 1)) & 0xFFFFFFFF, R) & mask)
        x = np.where(walking, (L << half) | R, x)
        walking &= x >= u(n)
    return x.astype(np.int64)


def test_sample_perm(got, recorded):
    _same(got, recorded, "sample_perm.", len(cases.PERM_CASES) * len(cases.PERM_SEEDS))
    for n, batch in cases.PERM_CASES:
        for seed in cases.PERM_SEEDS:
            assert np.array_equal(got[f"sample_perm.{n}.{batch}.{seed}"], feistel_perm(np.arange(batch), n, seed)), (n, batch, seed)


def test_raygen_fwd(got, recorded):
    _same(got, recorded, "raygen_fwd.", 2 * (1 + len(cases.FWD_COUNTS)))
    assert recorded["raygen_fwd.7x5.d"].shape == (35, 3) and recorded["raygen_fwd.40x30.257.o"].shape == (257, 3)


def test_gather_gt(got, recorded):
    _same(got, recorded, "gather_gt.", 2)
    assert not np.array_equal(recorded["gather_gt.3"], recorded["gather_gt.4"])


def test_raygen_bwd_in_one_workgroup(got, recorded):
    """n <= 256: one workgroup, one fixed order of its atomics.  (At 257 two workgroups add to every word in an order that is not
    fixed: tests/test_a_ops_gpu.py::test_raygen covers that size with its tolerance.)"""
    _same(got, recorded, "raygen_bwd.", 2 * len(cases.BWD_COUNTS))
    assert all(np.abs(recorded[f"raygen_bwd.{n}.d_pose"]).max() > 0 for n in cases.BWD_COUNTS)


def test_ray_batch_fwd(got, recorded):
    """Segments of 86 / 86 / 0 / 85 rays; injected pixels and the device draw; with images (pix, d, o, gt) and without (pix, d, o)."""
    _same(got, recorded, "ray_batch_fwd.", 2 * (4 + 3))
    for draw in ("injected", "drawn"):
        for key in ("pix", "d", "o"):       # the images change nothing but gt
            assert np.array_equal(got[f"ray_batch_fwd.{draw}.images.{key}"], got[f"ray_batch_fwd.{draw}.no_images.{key}"])
    drawn = got["ray_batch_fwd.drawn.images.pix"]
    for k, (lo, hi) in enumerate(zip(cases.SEG_START, cases.SEG_START[1:])):
        key = (cases.BATCH_SEED + k * 0x9E3779B9) & 0xFFFFFFFF
        assert np.array_equal(drawn[lo:hi], feistel_perm(np.arange(hi - lo), cases.BH * cases.BW, key)), k


def test_ray_batch_bwd(got, recorded):
    """Every segment <= 256 rays: one workgroup per segment.  With distinct cameras every word has one workgroup's atomics in their
    fixed order: bit equality.  Where camera 5 owns two segments, two workgroups add to its words: a word of d_kinv receives ONE
    value from each, and two contributions onto a zeroed word commute exactly: bit equality.  A word of that camera's d_pose
    receives two or three values from each workgroup (its own sum, and the origin terms of mcn_raygen_bwd_flush), four to six values
    in an order that is not fixed, so for those 12 words the gate is the one tests/test_multicam_gpu.py uses for unordered
    atomics, 16 * 2^-24 of the tensor's largest entry; every other camera's rows stay bit-equal."""
    _same(got, recorded, "ray_batch_bwd.distinct.", 2)
    _same(got, recorded, "ray_batch_bwd.shared.d_kinv", 1)
    new, old = got["ray_batch_bwd.shared.d_pose"], recorded["ray_batch_bwd.shared.d_pose"]
    shared = cases.SEG_CAMS["shared"][0]
    others = [c for c in range(cases.C) if c != shared]
    assert np.array_equal(new[others], old[others])
    err, big = float(np.abs(new[shared] - old[shared]).max()), float(np.abs(old).max())
    print(f"[ray_batch_bwd, camera in two segments] d_pose rows of that camera: max |new - recorded| {err:.3e}, max|recorded| {big:.3e}, "
          f"bit-equal: {np.array_equal(new[shared], old[shared])}")
    assert err <= 16.0 * 2.0 ** -24 * big
    unused = [c for c in range(cases.C) if c not in cases.SEG_CAMS["shared"]]
    assert np.abs(new[unused]).max() == 0.0 and np.abs(recorded["ray_batch_bwd.shared.d_kinv"][shared]).max() > 0


# ------------------------------------------------------------------------------------------------------------------ with the lens
# The two lens kernels against tests/golden/ray_preamble_lens.npz: the same batch with a fixed non-zero lens [7,2] (|k1| <= 0.08,
# |k2| <= 0.01), recorded on an MI355X from the library of the commit before the pinhole and the lens kernels became one body with a
# lens option (tests/golden/make_ray_preamble_lens.py; its recorder refused an inert lens: every non-empty segment's directions differ
# from the pinhole kernel's and every camera that owns rays has a non-zero d_lens row).
_spec = importlib.util.spec_from_file_location("make_ray_preamble_lens", os.path.join(GOLDEN, "make_ray_preamble_lens.py"))
lens_cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lens_cases)


@pytest.fixture(scope="module")
def lens_recorded(recorded):
    z = load_golden("ray_preamble_lens")
    z.update({k: v for k, v in recorded.items() if k.startswith("in.b_")})
    return z


@pytest.fixture(scope="module")
def lens_got(lens_recorded, gpu_device):
    """Every lens case, run once."""
    return lens_cases.run(lens_recorded, gpu_device)


def test_lens_ray_batch_fwd(lens_got, lens_recorded, recorded):
    """The cases of test_ray_batch_fwd at k != 0: bit equality; the pixels and origins are the pinhole kernel's, the directions are not."""
    _same(lens_got, lens_recorded, "lens_ray_batch_fwd.", 2 * (4 + 3))
    lens = lens_recorded["in.lens"]
    assert lens.shape == (cases.C, 2) and np.abs(lens[:, 0]).max() <= 0.08 and np.abs(lens[:, 1]).max() <= 0.01 and np.all(lens != 0)
    for draw in ("injected", "drawn"):
        for key in ("pix", "o", "gt"):
            for images in ("images", "no_images")[:1 if key == "gt" else 2]:
                assert np.array_equal(lens_recorded[f"lens_ray_batch_fwd.{draw}.{images}.{key}"], recorded[f"ray_batch_fwd.{draw}.{images}.{key}"])
        d, d0 = lens_recorded[f"lens_ray_batch_fwd.{draw}.images.d"], recorded[f"ray_batch_fwd.{draw}.images.d"]
        for lo, hi in zip(cases.SEG_START, cases.SEG_START[1:]):
            assert hi == lo or not np.array_equal(d[lo:hi], d0[lo:hi]), (draw, lo, hi)


def test_lens_ray_batch_bwd(lens_got, lens_recorded):
    """As test_ray_batch_bwd, with d_lens: distinct cameras, bit equality throughout.  Camera 5 in two segments: a word of d_kinv or
    d_lens receives ONE value from each of two workgroups onto a zeroed word, which commutes: bit equality; that camera's 12 d_pose
    words receive four to six values in an order that is not fixed: the gate of test_ray_batch_bwd, 16 * 2^-24 of the tensor's
    largest entry; every other camera's rows bit-equal, unused cameras exactly zero."""
    _same(lens_got, lens_recorded, "lens_ray_batch_bwd.distinct.", 3)
    _same(lens_got, lens_recorded, "lens_ray_batch_bwd.shared.d_kinv", 1)
    _same(lens_got, lens_recorded, "lens_ray_batch_bwd.shared.d_lens", 1)
    new, old = lens_got["lens_ray_batch_bwd.shared.d_pose"], lens_recorded["lens_ray_batch_bwd.shared.d_pose"]
    shared = cases.SEG_CAMS["shared"][0]
    others = [c for c in range(cases.C) if c != shared]
    assert np.array_equal(new[others], old[others])
    err, big = float(np.abs(new[shared] - old[shared]).max()), float(np.abs(old).max())
    print(f"[lens_ray_batch_bwd, camera in two segments] d_pose rows of that camera: max |new - recorded| {err:.3e}, max|recorded| {big:.3e}, "
          f"bit-equal: {np.array_equal(new[shared], old[shared])}")
    assert err <= 16.0 * 2.0 ** -24 * big
    for table, cams in cases.SEG_CAMS.items():
        unused = [c for c in range(cases.C) if c not in cams]
        for key in ("d_pose", "d_kinv", "d_lens"):
            assert np.abs(lens_got[f"lens_ray_batch_bwd.{table}.{key}"][unused]).max() == 0.0, (table, key)
        owners = sorted({c for c, lo, hi in zip(cams, cases.SEG_START, cases.SEG_START[1:]) if hi > lo})
        assert np.all(lens_recorded[f"lens_ray_batch_bwd.{table}.d_lens"][owners] != 0), table
