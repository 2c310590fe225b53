"""Per-ray sample bounds (sys_param key "ray_bounds"): what needs no GPU.

  the keys         "ray_bounds" is "global" (the default: today's model, nothing new in the state dict) or "aabb"; "ray_bounds_box" is six
                   finite numbers with every min below its max, by default the cube of boader_min / boader_max; every ValueError names
                   its key;
  refusals         a CPU model refuses an aabb render with McnerfError; the ops refuse host tensors before the library is opened; the
                   entry points refuse bad sizes, null pointers and bad boxes ahead of any device work;
  the header       include/mcnerf_box.h parses with the core header's parser, its names disjoint from the four other headers; one
                   build() call makes five libraries, the fifth exporting exactly its header and linking none of the core's objects;
                   with MCNBOX_LIB pointing nowhere default-key models are constructed without the library being opened;
  the restatement  tests/ray_bounds_ref.py: rows are non-decreasing and an unclipped ray's row is fl(g + jitter) bit for bit, on random
                   rays and boxes; the hand-made rays are clipped or not as their table says; the rays of the GPU model tests meet
                   their stated shares; the affine map against fp64 within the bound of the GPU test.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import ray_bounds_ref as B
from conftest import make_sys_param

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS, PDF, SELECT, UPDATE = "mcnerf_box_ray_depths", "mcnerf_box_sample_pdf_rows", "mcnerf_box_voxel_select_rows", "mcnerf_box_voxel_update_rows"


def _cfg():
    from oracle import mcnerf_oracle as O
    return O.RenderCfg(samples=16, scale=2, coarse=O.NetCfg(2, 32, (1,)), fine=O.NetCfg(2, 32, (1,)))


# ------------------------------------------------------------------------------------------------------------------ the keys
@pytest.mark.parametrize("bad", [True, None, "box", "AABB", 1, ["aabb"]])
def test_ray_bounds_must_be_global_or_aabb(bad):
    from mc_nerf_amd.model import NeRF_Model
    with pytest.raises(ValueError, match="ray_bounds"):
        NeRF_Model(make_sys_param(_cfg(), ray_bounds=bad))


@pytest.mark.parametrize("bad", [None, "cube", 3.5, (1, 2, 3), (0, 0, 0, 1, 1, 1, 1), (0, 0, 0, 1, 1, float("nan")), (0, 0, 0, 1, float("inf"), 1),
                                 (0, 0, 0, 1, 1, True), (0, 0, 0, 1, "1", 1), (0, 0, 0, 0, 1, 1), (0, 2, 0, 1, 1, 1), (0, 0, 1, 1, 1, 1 + 1e-9)])
def test_a_bad_box_names_its_key(bad):
    from mc_nerf_amd.model import NeRF_Model
    with pytest.raises(ValueError, match="ray_bounds_box"):
        NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", ray_bounds_box=bad))


def test_the_default_box_is_the_voxel_cube_and_its_keys_are_validated():
    from mc_nerf_amd.model import NeRF_Model
    m = NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb"))
    assert m.settings.aabb and m.settings.box == (-3.5, -3.5, -3.5, 3.5, 3.5, 3.5) and m.last_ray_span is None
    m = NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", ray_bounds_box=[-1, -1.5, -0.5, 1, 1.5, 2]))
    assert m.settings.box == (-1.0, -1.5, -0.5, 1.0, 1.5, 2.0)
    for key in ("boader_min", "boader_max"):
        sp = make_sys_param(_cfg(), ray_bounds="aabb")
        del sp[key]
        with pytest.raises(ValueError, match=key):
            NeRF_Model(sp)
        with pytest.raises(ValueError, match=key):
            NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", **{key: float("nan")}))
        NeRF_Model(dict(sp, ray_bounds_box=(0, 0, 0, 1, 1, 1)))          # with a box the cube's keys are not read
    with pytest.raises(ValueError, match="boader_min"):
        NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", boader_min=2.0, boader_max=2.0))


def test_the_default_is_todays_model():
    import dataclasses
    from mc_nerf_amd.model import NeRF_Model
    from mc_nerf_amd.model.render import RenderSettings
    off, glob, on = (NeRF_Model(make_sys_param(_cfg(), **kw)) for kw in ({}, dict(ray_bounds="global"), dict(ray_bounds="aabb")))
    for m in (off, glob):
        assert m.ray_bounds == "global" and not m.settings.aabb and m.settings.box is None and m.last_ray_span is None
    assert NeRF_Model(make_sys_param(_cfg(), ray_bounds_box="never read")).settings.box is None
    assert list(off.state_dict()) == list(on.state_dict())            # no new parameter, no new buffer
    fields = [f.name for f in dataclasses.fields(RenderSettings)]
    assert {"ray_bounds", "box"} <= set(fields) and RenderSettings(16, 2, 0.1, 0.0, True).ray_bounds == "global"


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_a_cpu_model_refuses_aabb_mode():
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import NeRF_Model
    m = NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb"))
    d = torch.nn.functional.normalize(torch.randn(4, 3), dim=-1)
    with pytest.raises(McnerfError, match="ray_bounds"):
        m.render_rays_train(d, -3.0 * d, 0, 1.0)
    with pytest.raises(McnerfError, match="ray_bounds"):
        m.render_rays_test(d, -3.0 * d, m.nerf_coarse, m.nerf_fine)


def test_bounds_ops_refuse_host_tensors_before_the_library_is_opened(monkeypatch):
    from mc_nerf_amd import _box, ops
    from mc_nerf_amd._lib import McnerfError
    monkeypatch.setattr(_box, "lib", lambda: pytest.fail("the library was opened"))
    o, d, g = torch.zeros(2, 3), torch.ones(2, 3), torch.linspace(1, 8, 4)
    with pytest.raises(McnerfError, match=DEPTHS + r": rays_o .*no CPU fallback"):
        ops.ray_depths(o, d, B.BOX, 1.0, 8.0, None, g)
    with pytest.raises(McnerfError, match="six numbers"):
        ops.ray_depths(o, d, B.BOX[:5], 1.0, 8.0, None, g)
    with pytest.raises(McnerfError, match="jitter"):
        ops.ray_depths(o, d, B.BOX, 1.0, 8.0, torch.zeros(3), g)
    rows = torch.ones(2, 4)
    with pytest.raises(McnerfError, match=PDF + r": w .*no CPU fallback"):
        ops.sample_pdf(torch.ones(2, 4), None, None, torch.rand(2, 5), z_rows=rows)
    with pytest.raises(McnerfError, match="z_rows"):
        ops.sample_pdf(torch.ones(2, 4), g, None, torch.rand(2, 5), z_rows=rows)
    with pytest.raises(McnerfError, match="z_rows"):
        ops.sample_pdf(torch.ones(2, 4), None, None, torch.rand(2, 5), z_rows=torch.ones(2, 5))
    grid = ops.VoxelGrid(2, -1.0, 1.0, 0.0, "cpu")
    with pytest.raises(McnerfError, match=SELECT + r": vox .*no CPU fallback"):
        ops.voxel_select(grid, 0.0, o, d, None, None, -20.0, z_rows=rows)
    with pytest.raises(McnerfError, match="z_rows"):
        ops.voxel_select(grid, 0.0, o, d, None, torch.zeros(2), -20.0, z_rows=rows)
    with pytest.raises(McnerfError, match=UPDATE + r": vox .*no CPU fallback"):
        ops.voxel_update(grid, 0.1, o, d, None, None, torch.zeros(2, 4, 4), z_rows=rows)
    with pytest.raises(McnerfError, match="z_rows"):
        ops.voxel_update(grid, 0.1, o, d, g, None, torch.zeros(2, 4, 4), z_rows=rows)


def test_entry_points_refuse_before_any_device_work():
    """Raw addresses that are never dereferenced: every refusal below is decided on the host (no GPU is needed)."""
    from mc_nerf_amd import _box
    from mc_nerf_amd._lib import McnerfError
    P = 4096                                # a non-null "pointer"
    inf, nan = float("inf"), float("nan")
    box = B.BOX
    _box.call(DEPTHS, None, None, 0, *box, 1.0, 8.0, None, None, 4, None, 0, None, None, None, 0)        # N = 0: no-ops, null pointers allowed
    _box.call(PDF, None, None, None, 0, 8, 4, None, 0)
    dep = lambda o=P, d=P, N=2, b=box, near=1.0, far=8.0, g=P, Sc=4, gf=P, Sf=8, zc=P, zf=P: (o, d, N, *b, near, far, None, g, Sc, gf, Sf, zc, zf, None, 0)
    sel = lambda vox=P, G=4, s=0.5, z=P, N=2, Sc=4, rc=P: (vox, G, -1.0, s, 0.0, P, P, z, N, Sc, -20.0, rc, P, P, P, None, 0)
    upd = lambda vox=P, G=4, s=0.5, z=P, N=2, Sc=4, idx=None, cnt=None, rows=0, sig=P: (vox, P, G, -1.0, s, 0.1, 0.9, P, P, z, N, Sc, idx, cnt, rows, sig, 0)
    bad = [
        (DEPTHS, dep(o=None)), (DEPTHS, dep(d=None)), (DEPTHS, dep(g=None)), (DEPTHS, dep(zc=None)),     # null required pointers
        (DEPTHS, dep(N=-1)), (DEPTHS, dep(Sc=0)), (DEPTHS, dep(Sf=-1)),
        (DEPTHS, dep(gf=None)), (DEPTHS, dep(zf=None)), (DEPTHS, dep(Sf=0)),                             # the second grid: all or none
        (DEPTHS, dep(N=1 << 21, Sc=1 << 10)), (DEPTHS, dep(N=1 << 21, Sf=1 << 10)),                      # N S >= 2^31
        (DEPTHS, dep(b=(0, 0, 0, 0, 1, 1))), (DEPTHS, dep(b=(0, 2, 0, 1, 1, 1))), (DEPTHS, dep(b=(0, 0, 0, 1, 1, nan))),
        (DEPTHS, dep(b=(-inf, 0, 0, 1, 1, 1))), (DEPTHS, dep(b=(0, 0, 0, 1, inf, 1))),
        (DEPTHS, dep(near=nan)), (DEPTHS, dep(far=inf)), (DEPTHS, dep(near=8.0)), (DEPTHS, dep(near=9.0)),
        (DEPTHS, dep(N=0, b=(0, 0, 0, 0, 1, 1))),                                                        # ... even with no rays
        (PDF, (P, P, P, 2, 2, 4, P, 0)), (PDF, (P, P, P, 2, 8, 0, P, 0)), (PDF, (P, P, P, 2, 1000, 25, P, 0)), (PDF, (P, P, P, -1, 8, 4, P, 0)),
        (PDF, (None, P, P, 2, 8, 4, P, 0)), (PDF, (P, None, P, 2, 8, 4, P, 0)), (PDF, (P, P, None, 2, 8, 4, P, 0)), (PDF, (P, P, P, 2, 8, 4, None, 0)),
        (PDF, (P, P, P, 1 << 22, 512, 512, P, 0)),
        (SELECT, sel(vox=None)), (SELECT, sel(G=1)), (SELECT, sel(G=1025)), (SELECT, sel(s=0.0)), (SELECT, sel(s=nan)), (SELECT, sel(z=None)),
        (SELECT, sel(N=-1)), (SELECT, sel(Sc=0)), (SELECT, sel(rc=None)), (SELECT, sel(N=1 << 21, Sc=1 << 10)),
        (UPDATE, upd(vox=None)), (UPDATE, upd(G=1)), (UPDATE, upd(s=inf)), (UPDATE, upd(z=None)), (UPDATE, upd(sig=None)), (UPDATE, upd(N=-1)),
        (UPDATE, upd(Sc=0)), (UPDATE, upd(idx=P)), (UPDATE, upd(cnt=P)), (UPDATE, upd(rows=-1)), (UPDATE, upd(N=1 << 21, Sc=1 << 10)),
    ]
    for name, args in bad:
        with pytest.raises(McnerfError, match=name + r" failed \(-1\): " + name + ": invalid argument"):
            _box.call(name, *args)


# ------------------------------------------------------------------------------------------------------------------ header / library
HEADERS = ("mcnerf.h", "mcnerf_ext.h", "mcnerf_reg.h", "mcnerf_geo.h", "mcnerf_box.h")


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(mcnerf_[a-z_0-9]+)\s*\(", text))


def test_the_bounds_header_parses_and_its_names_are_its_own():
    from ctypes import c_float, c_int, c_void_p
    from mc_nerf_amd import _box, _ext, _geo, _lib, _reg
    with open(os.path.join(ROOT, "include", "mcnerf_box.h")) as f:
        params, defines = _lib.parse_header(f.read())
    assert params == _box.PARAMS and defines == _box.DEFINES
    assert sorted(_box.SIGNATURES) == sorted(_declared("mcnerf_box.h")) and len(_box.SIGNATURES) == 6
    assert all(n.startswith("mcnerf_box_") for n in _box.SIGNATURES) and all(k.startswith("MCNERF_BOX_") for k in _box.DEFINES)
    assert _box.ABI_VERSION == 1
    for other in (_lib, _ext, _reg, _geo):
        assert not set(_box.SIGNATURES) & set(other.SIGNATURES) and not set(_box.DEFINES) & set(other.DEFINES)
    at = {p[0]: (p[2], p[3]) for p in _box.PARAMS[DEPTHS][1]}
    assert [p[0] for p in _box.PARAMS[DEPTHS][1]][3:9] == ["xmin", "ymin", "zmin", "xmax", "ymax", "zmax"] and at["zmax"] == (c_float, None)
    assert at["rays_o"] == (c_void_p, torch.float32) and at["span"] == (c_void_p, torch.float32) and at["Sf"] == (c_int, None)
    av = {p[0]: (p[2], p[3]) for p in _box.PARAMS[UPDATE][1]}
    assert av["scratch"] == (c_void_p, torch.int32) and av["idx"] == (c_void_p, torch.int32) and av["z_rows"] == (c_void_p, torch.float32)
    assert _box.McnerfError is _lib.McnerfError and _box.call not in (_lib.call, _ext.call, _reg.call, _geo.call)
    # the four pinned ABIs are what they were
    assert _lib.ABI_VERSION == 7 and len(_lib.SIGNATURES) == 53 and len(_ext.SIGNATURES) == 6 and len(_reg.SIGNATURES) == 4 and len(_geo.SIGNATURES) == 6


def test_a_missing_library_is_never_opened_by_default_key_models():
    env = dict(os.environ, MCNBOX_LIB="/nonexistent/libmcnbox.so", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    code = ("import mc_nerf_amd\n"
            "from mc_nerf_amd import _box, ops, synthetic as S\n"
            "from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, NeRF_Model\n"
            "assert _box.LIB_PATH == '/nonexistent/libmcnbox.so' and not _box.loaded()\n"
            "sp = S.make_sys_param('cpu', samples=8, scale=2, batch=16, H=8, W=8, coarse=(2, 32, [1]), fine=(2, 32, [1]))\n"
            "NeRF_Model(sp); MC_Model(sp); MC_NeRF_Loss(sp)\n"
            "NeRF_Model(dict(sp, ray_bounds='global')); NeRF_Model(dict(sp, ray_bounds='aabb'))\n"
            "assert not _box.loaded()\n"
            "try:\n    _box.call('mcnerf_box_sample_pdf_rows', None, None, None, 0, 8, 4, None, 0)\n"
            "except _box.McnerfError as e:\n    assert 'not found' in str(e) and 'no CPU fallback' in str(e)\n"
            "else:\n    raise SystemExit('a missing library did not raise')\n")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)


@pytest.fixture(scope="module")
def built():
    from mc_nerf_amd import build
    if not os.path.isfile(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    core = build.build(verbose=False)
    return core, build.EXT_OUT, build.REG_OUT, build.GEO_OUT, build.BOX_OUT


def test_one_build_call_makes_five_libraries(built):
    from mc_nerf_amd import _box, build
    assert built[0] == build.OUT and all(os.path.isfile(p) for p in built) and os.path.basename(built[4]) == "libmcnbox.so"
    assert build.BOX_SOURCES == ["box_api.hip", "ray_bounds.hip"]
    assert not set(build.BOX_SOURCES) & (set(build.SOURCES) | set(build.EXT_SOURCES) | set(build.REG_SOURCES) | set(build.GEO_SOURCES))
    assert all(os.path.isfile(os.path.join(build.CSRC, s)) for s in build.BOX_SOURCES + build.BOX_HEADERS)
    assert not any(s in build.FILE_FLAGS for s in build.BOX_SOURCES)
    # the sampler's and the voxel cell's device code reaches both libraries through headers both lists name
    for h in ("mcnerf_sample_pdf.h", "mcnerf_voxel.h", "mcnerf_compact.h", "mcnerf_maxkey.h"):
        assert h in build.HEADERS and h in build.BOX_HEADERS, h
    assert "voxel.hip" in build.BOX_HEADERS and '#include "voxel.hip"' in open(os.path.join(build.CSRC, "ray_bounds.hip")).read()
    l = _box.lib()
    assert l.mcnerf_box_abi_version() == _box.ABI_VERSION and l.mcnerf_box_last_error() is not None


def test_the_fifth_library_exports_its_own_header(built):
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    from mc_nerf_amd import _box
    sets = []
    for lib in built:
        out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
        sets.append({l.split()[-1] for l in out.splitlines() if l.strip() and l.split()[-1].startswith("mcnerf_")})
    assert sets[4] == _declared("mcnerf_box.h") == set(_box.SIGNATURES)
    for i in range(4):
        assert not sets[i] & sets[4], HEADERS[i]


def test_the_shared_device_code_is_defined_once():
    """The sampler's per-ray body, the voxel cell, predicate and item and the scan's body: one definition each (a definition is a line at
    column 0 that names the function before a `(` and is no declaration)."""
    from mc_nerf_amd import build
    once = {"mcn_sample_pdf_ray": "mcnerf_sample_pdf.h", "count_le": "mcnerf_sample_pdf.h", "vox_axis": "voxel.hip",
            "vox_cell": "voxel.hip", "vox_sample_cell": "voxel.hip", "vox_item": "voxel.hip",
            "mcn_scan_counts": "mcnerf_compact.h", "box_ray_span": "ray_bounds.hip"}
    defined = {name: [] for name in once}
    for fn in sorted(f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".h"))):
        text = open(os.path.join(build.CSRC, fn)).read()
        for line in text.split("\n"):
            code = re.sub(r"//.*", "", line).rstrip()
            for name in once:
                if re.match(rf"[A-Za-z_][^=;]*\b{name}\s*\(", code) and not code.endswith(";"):
                    defined[name].append(fn)
        if fn in build.BOX_SOURCES + ["mcnerf_sample_pdf.h", "mcnerf_ray_bounds.h"]:
            assert not re.findall(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", text, flags=re.M), fn
            assert "asm" not in re.sub(r"//.*", "", text), fn
    assert defined == {name: [fn] for name, fn in once.items()}
    assert "struct VoxelPred" in open(os.path.join(build.CSRC, "voxel.hip")).read()
    assert sum("struct VoxelPred" in open(os.path.join(build.CSRC, f)).read() for f in os.listdir(build.CSRC)) == 1


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_the_hand_made_rays_are_clipped_as_their_table_says():
    o, d = B.hand_rays(len(B.HAND))
    lo, hi, clipped = B.span_ref(o, d, B.BOX, B.NEAR, B.FAR)
    assert clipped.tolist() == [h[2] for h in B.HAND]
    assert bool((lo[~clipped] == B.NEAR).all()) and bool((hi[~clipped] == B.FAR).all())
    assert bool((lo[clipped] >= B.NEAR).all()) and bool((hi[clipped] <= B.FAR).all()) and bool((hi > lo).all())
    assert (float(lo[1]), float(lo[9]), float(hi[9])) == (B.NEAR, B.NEAR, B.FAR)          # origin inside; no axis constrains
    assert (float(lo[11]), float(hi[11]), float(lo[16]), float(hi[16])) == (3.0, 5.0, 1.0, float(torch.tensor(2.2)))
    lo13 = B.span_ref(o[13:14], d[13:14], B.BOX, 0.5, B.FAR)                                # the graze itself: t_in == t_out
    assert not bool(lo13[2]) and (float(lo13[0]), float(lo13[1])) == (0.5, B.FAR)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rows_are_non_decreasing_and_the_identity_on_unclipped_rays(seed):
    g = torch.Generator().manual_seed(seed)
    N = 4000
    o = torch.randn(N, 3, generator=g) * 3.0
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    d[torch.rand(N, 3, generator=g) < 0.05] = 0.0
    c, h = torch.randn(3, generator=g), torch.rand(3, generator=g) * 2.0 + 0.5
    box = tuple((c - h).tolist() + (c + h).tolist())
    for Sc, near, far in ((64, 1.0, 8.0), (65, 2.0, 6.0), (3, 0.05, 100.0)):
        grid = torch.linspace(near, far, Sc)
        jit = torch.rand(N, generator=g) * (far - near) / Sc
        for jitter in (jit, None):
            z, span, clipped = B.depths_ref(o, d, box, near, far, jitter, grid)
            assert 0.02 < float(clipped.float().mean()) < 0.98, float(clipped.float().mean())
            assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool(torch.isfinite(z).all())
            today = grid.unsqueeze(0).expand(N, -1) + (0.0 if jitter is None else jitter.unsqueeze(1))
            assert torch.equal(z[~clipped].view(torch.int32), today[~clipped].view(torch.int32))
            assert bool((span[~clipped] == torch.tensor([near, far])).all())
            # a box that clips nothing: every row is today's
            z_all = B.depths_ref(o, d, (-1e3,) * 3 + (1e3,) * 3, near, far, jitter, grid)[0]
            assert torch.equal(z_all.view(torch.int32), today.view(torch.int32))
            assert float((z - B.depths_exact(span, near, far, jitter, grid)).abs().max()) <= B.affine_bound(far, (far - near) / Sc)


def test_the_rays_of_the_gpu_model_tests_meet_their_shares():
    for N in (256, 512):
        d, o = B.model_rays(N)
        _, _, clipped = B.span_ref(o, d, B.BOX, B.NEAR, B.FAR)
        share = float(clipped.float().mean())
        assert 0.5 <= share <= 0.9 and int((~clipped).sum()) >= 1, share
        lo, hi, _ = B.span_ref(o, d, B.NO_CLIP, B.NEAR, B.FAR)             # the other box of those tests clips none of them
        assert bool((lo == B.NEAR).all()) and bool((hi == B.FAR).all())
    o, d = B.hand_rays(257)
    _, _, clipped = B.span_ref(o, d, B.BOX, B.NEAR, B.FAR)
    assert 0.3 < float(clipped.float().mean()) < 0.95
