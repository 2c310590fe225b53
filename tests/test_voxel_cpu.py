"""The voxel sigma cache (`coarse_sampler = "voxel"`) without a GPU: the four entry points in the header, the ctypes table and the
built library; the sys_param keys at model construction; the state-dict key set; the torch restatement (tests/voxel_ref.py) on grids
that can be checked by hand; the ops' refusal of CPU tensors."""
import os
import re

import pytest
import torch

import voxel_ref as V
from mc_nerf_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcnerf_voxel_select", "mcnerf_voxel_update", "mcnerf_voxel_query", "mcnerf_voxel_update_points"]
BMIN, BMAX = -3.5, 3.5


def _nerf(**kw):
    from mc_nerf_amd.model import NeRF_Model
    sp = S.make_sys_param("cpu", samples=32, scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    sp.update(kw)
    return NeRF_Model(sp)


def _rays(N, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    return d, -4.0 * d + 0.3 * torch.randn(N, 3, generator=g), g


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_declares_the_voxel_entry_points_and_keeps_its_version():
    import ctypes
    from mc_nerf_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "mcnerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in SYMBOLS:
        assert f"int {name}(" in code and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 7                             # (new symbols only; tests/test_abi_cpu.py checks header, table and library)


def test_voxel_source_is_in_the_build():
    from mc_nerf_amd import build
    assert "voxel.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "voxel.hip"))


# ------------------------------------------------------------------------------------------------------------------ the keys
def test_voxel_keys_reach_the_settings():
    m = _nerf()
    assert m.settings.coarse_sampler == "dense" and not m.settings.voxel and m.sigma_voxels is None and m.last_coarse_selection is None
    m = _nerf(coarse_sampler="voxel", grid_nerf=16)
    st = m.settings
    assert st.voxel and (st.voxel_beta, st.voxel_thresh, st.voxel_warmup_epoch) == (0.1, 0.0, 1) and m.grid_nerf == 16
    m = _nerf(coarse_sampler="voxel", grid_nerf=2, voxel_beta=1, voxel_thresh=-3.0, voxel_warmup_epoch=0)
    assert (m.settings.voxel_beta, m.settings.voxel_thresh, m.settings.voxel_warmup_epoch) == (1.0, -3.0, 0)
    assert _nerf(coarse_sampler="voxel", grid_nerf=1024).grid_nerf == 1024


@pytest.mark.parametrize("kw, key", [(dict(voxel_beta=0.0), "voxel_beta"), (dict(voxel_beta=1.5), "voxel_beta"), (dict(voxel_beta=-0.1), "voxel_beta"),
                                     (dict(voxel_beta="0.1"), "voxel_beta"), (dict(voxel_beta=float("nan")), "voxel_beta"),
                                     (dict(voxel_thresh=None), "voxel_thresh"), (dict(voxel_thresh=float("inf")), "voxel_thresh"),
                                     (dict(voxel_warmup_epoch=-1), "voxel_warmup_epoch"), (dict(voxel_warmup_epoch=2.5), "voxel_warmup_epoch"),
                                     (dict(voxel_warmup_epoch=True), "voxel_warmup_epoch"),
                                     (dict(grid_nerf=1), "grid_nerf"), (dict(grid_nerf=1025), "grid_nerf"), (dict(grid_nerf=64.0), "grid_nerf"),
                                     (dict(boader_min=3.5), "boader_min"), (dict(boader_min=1.0, boader_max=-1.0), "boader_min"),
                                     (dict(coarse_sampler="grid"), "coarse_sampler"), (dict(coarse_sampler=None), "coarse_sampler")])
def test_bad_voxel_settings_are_refused(kw, key):
    with pytest.raises(ValueError, match=key):
        _nerf(**{"coarse_sampler": "voxel", **kw})


def test_dense_mode_ignores_garbage_in_the_voxel_keys():
    garbage = dict(voxel_beta=-7, voxel_thresh="x", voxel_warmup_epoch=None, grid_nerf=-1, boader_min=9.0, boader_max=-9.0, sigma_init="?")
    for kw in (garbage, {"coarse_sampler": "dense", **garbage}):
        m = _nerf(**kw)
        assert m.settings.coarse_sampler == "dense" and m.sigma_voxels is None and m._voxels is None


def test_state_dict_keys_are_the_dense_models():
    dense, voxel = _nerf(), _nerf(coarse_sampler="voxel", grid_nerf=4)
    assert voxel.sigma_voxels.shape == (4, 4, 4) and bool((voxel.sigma_voxels == 30.0).all())       # allocated: still no buffer
    assert list(voxel.state_dict()) == list(dense.state_dict())
    assert [n for n, _ in voxel.named_buffers()] == [n for n, _ in dense.named_buffers()]
    assert [n for n, _ in voxel.named_parameters()] == [n for n, _ in dense.named_parameters()]


# ---------------------------------------------------------------------------------------------------------- the restatement
def test_cell_of_clamps_and_sends_nan_to_cell_zero():
    G = 4                                                               # cells of width 1.75 over [-3.5, 3.5]
    pts = torch.tensor([[-3.5, -3.5, -3.5], [3.49, 3.49, 3.49], [3.5, 3.5, 3.5], [-99.0, 99.0, 0.0], [float("nan"), 0.0, float("inf")],
                        [-1.75, 0.0, 1.75], [float("-inf"), -1.76, 1.74]])
    want = [(0, 0, 0), (3, 3, 3), (3, 3, 3), (0, 3, 2), (0, 2, 3), (1, 2, 3), (0, 0, 2)]
    assert V.cell_of(pts, G, BMIN, BMAX).tolist() == [(x * G + y) * G + z for x, y, z in want]
    assert float(V.scale_of(384, BMIN, BMAX)) == float(torch.tensor(384.0) / torch.tensor(7.0))


def test_fresh_grid_lists_every_pair_in_row_major_order_and_a_negative_grid_none():
    N, Sc, G = 9, 5, 4
    d, o, g = _rays(N, 1)
    z = torch.linspace(1.0, 8.0, Sc)
    jit = torch.rand(N, generator=g)
    idx, out_c = V.select(torch.full((G, G, G), 30.0), 0.0, o, d, z, jit, BMIN, BMAX, -20.0)
    assert torch.equal(idx, torch.stack(torch.meshgrid(torch.arange(N), torch.arange(Sc), indexing="ij"), -1).reshape(-1, 2))
    assert out_c.shape == (N, Sc, 4) and bool((out_c[..., 0] == -20.0).all()) and bool((out_c[..., 1:] == 1.0).all())
    idx, _ = V.select(torch.full((G, G, G), -1.0), 0.0, o, d, z, jit, BMIN, BMAX, -20.0)
    assert idx.shape == (0, 2)
    idx, _ = V.select(torch.zeros(G, G, G), 0.0, o, d, z, None, BMIN, BMAX, -20.0)          # occupied means V > thresh, strictly
    assert idx.shape == (0, 2)
    vox = torch.full((G, G, G), -1.0)
    vox[1, 2, 3] = 0.5                                                   # one occupied cell: exactly the samples inside it
    cells = V.sample_cells(o, d, z, jit, G, BMIN, BMAX)
    idx, _ = V.select(vox, 0.0, o, d, z, jit, BMIN, BMAX, -20.0)
    assert torch.equal(idx, torch.nonzero(cells == (1 * G + 2) * G + 3))


def test_update_with_beta_one_writes_the_per_cell_maximum():
    G = 4
    vox = torch.full((G, G, G), 30.0)
    pts = torch.tensor([[-3.0, -3.0, -3.0], [-2.9, -3.1, -3.2], [3.0, 3.0, 3.0], [-3.0, -3.0, -3.0], [0.1, 0.1, 0.1], [0.2, 0.2, 0.2]])
    sig = torch.tensor([-2.0, 1.5, float("nan"), -7.0, float("inf"), -0.25])
    new = V.update_points(vox, pts, sig, 1.0, BMIN, BMAX)
    assert float(new[0, 0, 0]) == 1.5 and float(new[2, 2, 2]) == -0.25
    assert float(new[3, 3, 3]) == 30.0                                   # its only sample is NaN: untouched
    touched = torch.zeros(G, G, G, dtype=torch.bool)
    touched[0, 0, 0] = touched[2, 2, 2] = True
    assert torch.equal(new[~touched], vox[~touched]) and bool((vox == 30.0).all())
    half = V.update_points(vox, pts, sig, 0.5, BMIN, BMAX)
    assert float(half[0, 0, 0]) == 0.5 * 30.0 + 0.5 * 1.5
    assert torch.equal(V.query(new, pts, BMIN, BMAX), torch.tensor([1.5, 1.5, 30.0, 1.5, -0.25, -0.25]))


def test_key_round_trips_and_orders_floats():
    v = torch.tensor([-3.0e38, -1.0, -1e-30, -0.0, 0.0, 1e-30, 1.0, 3.0e38])
    k = V._key(v)
    assert bool((k[1:] > k[:-1]).all()) and int(k.min()) > 0 and int(k.max()) < 1 << 32
    assert torch.equal(V._unkey(k).view(torch.int32), v.view(torch.int32))


def test_centres_are_the_cell_midpoints():
    c = V.centres(4, BMIN, BMAX)
    assert c.shape == (4, 4, 4, 3) and c[1, 2, 3].tolist() == [-0.875, 0.875, 2.625]
    assert torch.equal(V.cell_of(c.reshape(-1, 3), 4, BMIN, BMAX), torch.arange(64))


# ---------------------------------------------------------------------------------------------------------------- CPU tensors
def test_voxel_ops_refuse_cpu_tensors():
    from mc_nerf_amd import _lib, ops
    grid = ops.VoxelGrid(4, BMIN, BMAX, 30.0, "cpu")
    d, o, _ = _rays(8, 2)
    z = torch.linspace(1.0, 8.0, 16)
    with pytest.raises(_lib.McnerfError):
        ops.voxel_select(grid, 0.0, o, d, z, None, -20.0)
    with pytest.raises(_lib.McnerfError):
        ops.voxel_update(grid, 0.1, o, d, z, None, torch.zeros(8, 16, 4))
    with pytest.raises(_lib.McnerfError):
        ops.voxel_query(grid, o)
    with pytest.raises(_lib.McnerfError):
        ops.voxel_update_points(grid, o, torch.zeros(8), 0.1)
    m = _nerf(coarse_sampler="voxel", grid_nerf=4)
    with pytest.raises(_lib.McnerfError):
        m.query_sigma(o)
    with pytest.raises(_lib.McnerfError):
        m.update_sigma(o, torch.zeros(8), 0.1)
    with pytest.raises(_lib.McnerfError):
        m.rebuild_voxels()
    with pytest.raises(_lib.McnerfError):
        _nerf().query_sigma(o)                                           # dense mode has no grid
