"""The scene box fitted to the voxel sigma cache (sys_param key "ray_bounds_fit"): what needs no GPU.

  the keys         "ray_bounds_fit" is "fixed" (the default: aabb mode as it was) or "voxel", which needs coarse_sampler = "voxel";
                   "ray_bounds_fit_margin" is an int >= 0 (2), "ray_bounds_fit_every" an int >= 1 (16); a bad value is a ValueError naming
                   the key; in "global" mode none of them is read; the state dict is what it was;
  the header       include/mcnerf_fit.h parses with the core header's parser, its names disjoint from the six other headers; the six
                   pinned ABIs are what they were; one build() call makes seven libraries, build.LIBRARIES still holding six, the
                   seventh exporting exactly its header;
  first use        with MCNFIT_LIB pointing nowhere, default-key, "fixed" and even "voxel" models are constructed without the library
                   being opened, and a direct call raises "not found ... no CPU fallback";
  refusals         a CPU model refuses a fit-mode render with McnerfError; the ops refuse host tensors before the library is opened; an
                   N = 0 call is a no-op on null pointers; bad sizes, null pointers and bad boxes are refused ahead of any device work;
  the restatement  tests/scene_fit_ref.py gives the boxes its table says on hand-made grids;
  the sources      no preprocessor conditional, no inline assembly, no restated shared body; the MLP source digest is unchanged.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import ray_bounds_ref as B
import scene_fit_ref as F
from conftest import make_sys_param

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX, DEPTHS = "mcnerf_fit_voxel_box", "mcnerf_fit_ray_depths"
HEADERS = ("mcnerf.h", "mcnerf_ext.h", "mcnerf_reg.h", "mcnerf_geo.h", "mcnerf_box.h", "mcnerf_hit.h", "mcnerf_fit.h")
VOXEL = dict(coarse_sampler="voxel", grid_nerf=16)


def _cfg():
    from oracle import mcnerf_oracle as O
    return O.RenderCfg(samples=16, scale=2, coarse=O.NetCfg(2, 32, (1,)), fine=O.NetCfg(2, 32, (1,)))


# ------------------------------------------------------------------------------------------------------------------ the keys
def test_the_default_is_fixed_and_voxel_is_accepted():
    import dataclasses
    from mc_nerf_amd.model import NeRF_Model
    from mc_nerf_amd.model.render import RenderSettings
    off, fixed, fit = (NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", **VOXEL, **kw))
                       for kw in ({}, dict(ray_bounds_fit="fixed"), dict(ray_bounds_fit="voxel")))
    for m in (off, fixed):
        st = m.settings
        assert st.ray_bounds_fit == "fixed" and st.aabb and not st.fit_box and m.scene_box is None and m.scene_cells is None
        assert (st.ray_bounds_fit_margin, st.ray_bounds_fit_every) == (2, 16) and m.last_scene_box is None
    st = fit.settings
    assert st.ray_bounds_fit == "voxel" and st.fit_box and (st.ray_bounds_fit_margin, st.ray_bounds_fit_every) == (2, 16)
    assert st.box == (-3.5,) * 3 + (3.5,) * 3 and fit.last_scene_box is None          # the outer box: the cube
    m = NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", ray_bounds_box=B.BOX, ray_bounds_fit="voxel", ray_bounds_fit_margin=0,
                                  ray_bounds_fit_every=1, **VOXEL))
    assert m.settings.box == tuple(float(torch.tensor(v)) for v in B.BOX)           # ... or the user's box
    assert (m.settings.ray_bounds_fit_margin, m.settings.ray_bounds_fit_every) == (0, 1)
    # no new parameter, no new buffer; until the first fit the box is the outer box and the cells say "nothing fitted"
    assert list(off.state_dict()) == list(fit.state_dict())
    cells, box = fit.scene_buffers()                                  # ops.voxel_box's order
    assert box.tolist() == list(st.box) and cells.tolist() == [16, 16, 16, -1, -1, -1, 0, 0] and fit.scene_box_status() == 0
    assert fit.scene_box is box and fit.scene_cells is cells and fit.scene_buffers()[1] is box
    assert list(off.state_dict()) == list(fit.state_dict()) and not any(b is box or b is cells for b in fit.buffers())
    fields = [f.name for f in dataclasses.fields(RenderSettings)]
    assert {"ray_bounds_fit", "ray_bounds_fit_margin", "ray_bounds_fit_every"} <= set(fields) and fields[-1] == "want_zexp"
    assert RenderSettings(16, 2, 0.1, 0.0, True).ray_bounds_fit == "fixed"
    assert not RenderSettings(16, 2, 0.1, 0.0, True, ray_bounds_fit="voxel").fit_box        # "global": the key changes nothing


@pytest.mark.parametrize("key, bad", [("ray_bounds_fit", b) for b in (True, None, "Voxel", "grid", 1, ["voxel"])]
                         + [("ray_bounds_fit_margin", b) for b in (-1, 1.0, True, None, "2")]
                         + [("ray_bounds_fit_every", b) for b in (0, -3, 2.0, False, None, "16")])
def test_a_bad_value_names_the_key(key, bad):
    from mc_nerf_amd.model import NeRF_Model
    kw = {"ray_bounds_fit": "voxel", key: bad}
    with pytest.raises(ValueError, match=key):
        NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", **VOXEL, **kw))


def test_voxel_without_the_voxel_cache_is_refused():
    from mc_nerf_amd.model import NeRF_Model
    for kw in ({}, dict(coarse_sampler="dense")):
        with pytest.raises(ValueError, match="ray_bounds_fit"):
            NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", ray_bounds_fit="voxel", **kw))
    NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", ray_bounds_fit="fixed"))           # "fixed" needs no cache


@pytest.mark.parametrize("value", ["voxel", "never read", None, 7])
def test_the_keys_are_never_read_in_global_mode(value):
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import NeRF_Model
    for kw in ({}, dict(ray_bounds="global")):
        m = NeRF_Model(make_sys_param(_cfg(), ray_bounds_fit=value, ray_bounds_fit_margin=value, ray_bounds_fit_every=value, **kw))
        st = m.settings
        assert (st.ray_bounds_fit, st.ray_bounds_fit_margin, st.ray_bounds_fit_every) == ("fixed", 2, 16) and not st.fit_box
        assert m.scene_box is None and m.scene_cells is None and m.last_scene_box is None
        with pytest.raises(McnerfError, match="ray_bounds_fit"):
            m.refit_scene_box()


# ------------------------------------------------------------------------------------------------------------------ header / library
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(mcnerf_[a-z_0-9]+)\s*\(", text))


def test_the_fit_header_parses_and_its_names_are_its_own():
    from ctypes import c_float, c_int, c_void_p
    from mc_nerf_amd import _box, _ext, _fit, _geo, _hit, _lib, _reg
    with open(os.path.join(ROOT, "include", "mcnerf_fit.h")) as f:
        params, defines = _lib.parse_header(f.read())
    assert params == _fit.PARAMS and defines == _fit.DEFINES
    assert sorted(_fit.SIGNATURES) == sorted(_declared("mcnerf_fit.h")) and len(_fit.SIGNATURES) == 4
    assert set(_fit.SIGNATURES) == {"mcnerf_fit_abi_version", "mcnerf_fit_last_error", BOX, DEPTHS}
    assert all(n.startswith("mcnerf_fit_") for n in _fit.SIGNATURES) and all(k.startswith("MCNERF_FIT_") for k in _fit.DEFINES)
    assert _fit.ABI_VERSION == 1
    for other in (_lib, _ext, _reg, _geo, _box, _hit):
        assert not set(_fit.SIGNATURES) & set(other.SIGNATURES) and not set(_fit.DEFINES) & set(other.DEFINES)
    # the depths: mcnerf_hit_ray_depths' list with the six box floats replaced by one pointer
    names = lambda b, fn: [p[0] for p in b.PARAMS[fn][1]]
    theirs = names(_hit, "mcnerf_hit_ray_depths")
    assert theirs[3:9] == ["xmin", "ymin", "zmin", "xmax", "ymax", "zmax"] and names(_fit, DEPTHS) == theirs[:3] + ["box"] + theirs[9:]
    assert names(_fit, BOX) == ["vox", "G", "bmin", "h", "thresh", "margin", "xmin", "ymin", "zmin", "xmax", "ymax", "zmax", "cells", "box", "stream"]
    at = lambda fn: {p[0]: (p[2], p[3]) for p in _fit.PARAMS[fn][1]}
    assert at(DEPTHS)["box"] == (c_void_p, torch.float32) and at(DEPTHS)["hit"] == (c_void_p, torch.int32)
    assert at(BOX)["cells"] == (c_void_p, torch.int32) and at(BOX)["box"] == (c_void_p, torch.float32) and at(BOX)["vox"] == (c_void_p, torch.float32)
    assert at(BOX)["margin"] == (c_int, None) and at(BOX)["h"] == (c_float, None)
    assert _fit.McnerfError is _lib.McnerfError and _fit.call not in (_lib.call, _ext.call, _reg.call, _geo.call, _box.call, _hit.call)
    text = open(os.path.join(ROOT, "mc_nerf_amd", "_fit.py")).read()
    assert "def " not in text and "CDLL" not in text and text.count("Binding(") == 1
    # the six pinned ABIs are what they were
    assert _lib.ABI_VERSION == 7 and [len(b.SIGNATURES) for b in (_lib, _ext, _reg, _geo, _box, _hit)] == [53, 6, 4, 6, 6, 6]
    assert _box.ABI_VERSION == 1 and _hit.ABI_VERSION == 1


def test_a_missing_library_is_opened_by_no_constructor():
    env = dict(os.environ, MCNFIT_LIB="/nonexistent/libmcnfit.so", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    code = ("import mc_nerf_amd\n"
            "from mc_nerf_amd import _fit, ops, synthetic as S\n"
            "from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, NeRF_Model\n"
            "assert _fit.LIB_PATH == '/nonexistent/libmcnfit.so' and not _fit.loaded()\n"
            "sp = S.make_sys_param('cpu', samples=8, scale=2, batch=16, H=8, W=8, coarse=(2, 32, [1]), fine=(2, 32, [1]))\n"
            "NeRF_Model(sp); MC_Model(sp); MC_NeRF_Loss(sp)\n"
            "NeRF_Model(dict(sp, ray_bounds='global', ray_bounds_fit='voxel')); NeRF_Model(dict(sp, ray_bounds='aabb'))\n"
            "NeRF_Model(dict(sp, ray_bounds='aabb', ray_bounds_fit='fixed')); MC_Model(dict(sp, ray_bounds='aabb', ray_bounds_fit='fixed'))\n"
            "vox = dict(sp, ray_bounds='aabb', ray_bounds_fit='voxel', coarse_sampler='voxel', grid_nerf=8)\n"
            "m = NeRF_Model(vox); MC_Model(vox); m.scene_buffers()\n"
            "assert not _fit.loaded()\n"
            "try:\n    _fit.call('mcnerf_fit_ray_depths', None, None, 0, None, 1.0, 8.0, None, None, 4, None, 0, None, None, None, None, 0)\n"
            "except _fit.McnerfError as e:\n    assert 'not found' in str(e) and 'no CPU fallback' in str(e)\n"
            "else:\n    raise SystemExit('a missing library did not raise')\n")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)


@pytest.fixture(scope="module")
def built():
    from mc_nerf_amd import build
    if not os.path.isfile(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    core = build.build(verbose=False)
    return core, build.EXT_OUT, build.REG_OUT, build.GEO_OUT, build.BOX_OUT, build.HIT_OUT, build.FIT_OUT


def test_one_build_call_makes_seven_libraries(built):
    from mc_nerf_amd import _fit, build
    assert built[0] == build.OUT and all(os.path.isfile(p) for p in built) and os.path.basename(built[6]) == "libmcnfit.so"
    assert len(build.LIBRARIES) == 6 and list(build.LIBRARIES)[-1] == "" and "FIT_" not in build.LIBRARIES
    assert list(build.EXTRA_LIBRARIES) == ["FIT_"] and build.EXTRA_LIBRARIES["FIT_"] == ("libmcnfit.so", build.FIT_SOURCES, build.FIT_HEADERS)
    assert build.FIT_SOURCES == ["fit_api.hip", "scene_fit.hip"]
    others = set(build.SOURCES) | set(build.EXT_SOURCES) | set(build.REG_SOURCES) | set(build.GEO_SOURCES) | set(build.BOX_SOURCES) | set(build.HIT_SOURCES)
    assert not set(build.FIT_SOURCES) & others
    assert all(os.path.isfile(os.path.join(build.CSRC, s)) for s in build.FIT_SOURCES + build.FIT_HEADERS)
    assert not any(s in build.FILE_FLAGS for s in build.FIT_SOURCES) and not any(f.startswith("-D") for f in build.FLAGS)
    # what scene_fit.hip compiles into the library by inclusion is listed with its headers, and so is the preamble
    assert '#include "ray_bounds.hip"' in open(os.path.join(build.CSRC, "scene_fit.hip")).read()
    for h in ("ray_bounds.hip", "select.hip", "voxel.hip", "mcnerf_compact.h", "mcnerf_ray_bounds.h", "mcnerf_scene_fit.h", "mcnerf_api.h", "mcnerf_multicam.h"):
        assert h in build.FIT_HEADERS, h
    l = _fit.lib()
    assert l.mcnerf_fit_abi_version() == _fit.ABI_VERSION and l.mcnerf_fit_last_error() is not None


def test_the_seventh_library_exports_its_own_header(built):
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    from mc_nerf_amd import _fit
    sets = []
    for lib in built:
        out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
        sets.append({l.split()[-1] for l in out.splitlines() if l.strip() and l.split()[-1].startswith("mcnerf_")})
    assert sets[6] == _declared("mcnerf_fit.h") == set(_fit.SIGNATURES)
    for i in range(6):
        assert not sets[i] & sets[6], HEADERS[i]
        assert sets[i] == _declared(HEADERS[i]), HEADERS[i]            # ... and the six others export what they did


def test_the_new_sources_restate_no_shared_body_and_have_no_switches():
    """The fit library's own files define none of the bodies it shares (a definition is a line at column 0 that names the function before
    a `(` and is no declaration), hold no preprocessor conditional and no inline assembly; the per-ray body of the depths is one device
    function of ray_bounds.hip that both kernels call."""
    import bench
    from mc_nerf_amd import build
    shared = ("box_ray_span", "ray_depths_kernel", "ray_depths_ray", "vox_sample_cell", "vox_cell", "vox_axis", "mcn_scan_counts", "mcn_launch_ray_depths")
    for fn in ("scene_fit.hip", "fit_api.hip", "mcnerf_scene_fit.h"):
        text = open(os.path.join(build.CSRC, fn)).read()
        code = re.sub(r"//.*", "", text)
        assert not re.findall(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", text, flags=re.M), fn
        assert "asm" not in code and "struct VoxelPred" not in code and "struct SelectPred" not in code, fn
        assert "atomicAdd" not in code and "atomicExch" not in code and "atomicCAS" not in code, fn       # integer min / max only
        assert "__fdiv_rn" not in code and "zgrid_c[" not in code, fn                                       # nothing of the slab test or the rows
        for line in code.split("\n"):
            for name in shared:
                assert not (re.match(rf"[A-Za-z_][^=;]*\b{name}\s*\(", line) and not line.rstrip().endswith(";")), (fn, name)
    src = {f: open(os.path.join(build.CSRC, f)).read() for f in os.listdir(build.CSRC)}
    assert [f for f, s in src.items() if "void ray_depths_ray(" in s] == ["ray_bounds.hip"]
    assert src["ray_bounds.hip"].count("ray_depths_ray(a);") == 1 and src["scene_fit.hip"].count("ray_depths_ray(a);") == 1
    assert sorted(f for f, s in src.items() if "ray_depths_ray(" in re.sub(r"//.*", "", s)) == ["ray_bounds.hip", "scene_fit.hip"]
    assert sum("struct VoxelPred" in s for s in src.values()) == 1 and "struct VoxelPred" in src["voxel.hip"]
    # nothing was added to the two headers of the MLP source digest, which is what it was
    for h in ("mcnerf_kernels.h", "mcnerf_common.h"):
        assert "Fit" not in src[h] and "fit_" not in src[h], h
    assert bench.csrc_digest() == "7c1c6a7b8f60d22d"


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_a_cpu_model_refuses_a_fit_mode_render():
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import NeRF_Model
    m = NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", ray_bounds_fit="voxel", voxel_warmup_epoch=5, **VOXEL))
    d = torch.nn.functional.normalize(torch.randn(4, 3), dim=-1)
    with pytest.raises(McnerfError, match="ray_bounds"):
        m.render_rays_train(d, -3.0 * d, 0, 1.0)
    with pytest.raises(McnerfError, match="ray_bounds"):
        m.render_rays_train(d, -3.0 * d, 9, 1.0)                      # (past the warm-up: refused ahead of the refit)
    with pytest.raises(McnerfError, match="ray_bounds"):
        m.render_rays_test(d, -3.0 * d, m.nerf_coarse, m.nerf_fine)
    with pytest.raises(McnerfError, match=BOX + r": vox .*no CPU fallback"):
        m.refit_scene_box()


def test_fit_ops_refuse_host_tensors_before_the_library_is_opened(monkeypatch):
    from mc_nerf_amd import _fit, ops
    from mc_nerf_amd._lib import McnerfError
    monkeypatch.setattr(_fit._B, "lib", lambda: pytest.fail("the library was opened"))      # (the instance's: `_fit.call` is its bound method and calls self.lib())
    o, d, g = torch.zeros(2, 3), torch.ones(2, 3), torch.linspace(1, 8, 4)
    box = torch.tensor(B.BOX)
    for want_hit in (False, True):
        with pytest.raises(McnerfError, match=DEPTHS + r": rays_o .*no CPU fallback"):
            ops.ray_depths(o, d, box, 1.0, 8.0, None, g, want_hit=want_hit)
    with pytest.raises(McnerfError, match="a box of six numbers"):
        ops.ray_depths(o, d, torch.zeros(5), 1.0, 8.0, None, g)
    grid = ops.VoxelGrid(4, -1.0, 1.0, 0.0, "cpu")
    assert grid.h == F.cell_edge(4, -1.0, 1.0) == 0.5
    with pytest.raises(McnerfError, match=BOX + r": vox .*no CPU fallback"):
        ops.voxel_box(grid, 0.0, 2, B.BOX)
    for bad in (dict(outer=B.BOX[:5]), dict(margin=1.0), dict(margin=True), dict(cells=torch.zeros(7, dtype=torch.int32)), dict(box=torch.zeros(7))):
        with pytest.raises(McnerfError, match="voxel_box: "):
            ops.voxel_box(grid, 0.0, **{"margin": 2, "outer": B.BOX, **bad})


def test_entry_points_refuse_before_any_device_work():
    """Raw addresses that are never dereferenced: every refusal below is decided on the host (no GPU is needed)."""
    from mc_nerf_amd import _fit
    from mc_nerf_amd._lib import McnerfError
    P = 4096                                # a non-null "pointer"
    inf, nan = float("inf"), float("nan")
    # N = 0: a no-op, null pointers allowed -- the box among them
    _fit.call(DEPTHS, None, None, 0, None, 1.0, 8.0, None, None, 4, None, 0, None, None, None, None, 0)
    dep = lambda o=P, d=P, N=2, b=P, near=1.0, far=8.0, g=P, Sc=4, gf=P, Sf=8, zc=P, zf=P: (o, d, N, b, near, far, None, g, Sc, gf, Sf, zc, zf, None, None, 0)
    fit = lambda vox=P, G=4, bmin=-1.0, h=0.5, thresh=0.0, margin=2, b=B.BOX, cells=P, box=P: (vox, G, bmin, h, thresh, margin, *b, cells, box, 0)
    bad = [
        (DEPTHS, dep(o=None)), (DEPTHS, dep(d=None)), (DEPTHS, dep(b=None)), (DEPTHS, dep(g=None)), (DEPTHS, dep(zc=None)),
        (DEPTHS, dep(N=-1)), (DEPTHS, dep(Sc=0)), (DEPTHS, dep(Sf=-1)), (DEPTHS, dep(gf=None)), (DEPTHS, dep(zf=None)), (DEPTHS, dep(Sf=0)),
        (DEPTHS, dep(N=1 << 21, Sc=1 << 10)), (DEPTHS, dep(N=1 << 21, Sf=1 << 10)),
        (DEPTHS, dep(near=nan)), (DEPTHS, dep(far=inf)), (DEPTHS, dep(near=8.0)), (DEPTHS, dep(N=0, near=8.0)), (DEPTHS, dep(N=0, Sc=0)),
        (BOX, fit(vox=None)), (BOX, fit(cells=None)), (BOX, fit(box=None)), (BOX, fit(G=1)), (BOX, fit(G=1025)), (BOX, fit(G=-4)),
        (BOX, fit(h=0.0)), (BOX, fit(h=-0.5)), (BOX, fit(h=nan)), (BOX, fit(h=inf)), (BOX, fit(bmin=nan)), (BOX, fit(thresh=nan)), (BOX, fit(margin=-1)),
        (BOX, fit(b=(0, 0, 0, 0, 1, 1))), (BOX, fit(b=(0, 2, 0, 1, 1, 1))), (BOX, fit(b=(0, 0, 0, 1, 1, nan))), (BOX, fit(b=(-inf, 0, 0, 1, 1, 1))),
    ]
    for name, args in bad:
        with pytest.raises(McnerfError, match=name + r" failed \(-1\): " + name + ": invalid argument"):
            _fit.call(name, *args)


# ------------------------------------------------------------------------------------------------------------------ the restatement
G8, BMIN8, H8 = 8, -2.0, 0.5                                # cells [-2 + 0.5 i, -2 + 0.5 (i + 1)]: every bound is exact in fp32
CUBE8 = (-2.0,) * 3 + (2.0,) * 3
TABLE = [
    # (occupied cells, margin, outer box) -> (cells[0:7], box)
    ([], 2, CUBE8, (8, 8, 8, -1, -1, -1, 0), CUBE8),
    ([(3, 4, 5)], 0, CUBE8, (3, 4, 5, 3, 4, 5, 1), (-0.5, 0.0, 0.5, 0.0, 0.5, 1.0)),
    ([(3, 4, 5)], 1, CUBE8, (3, 4, 5, 3, 4, 5, 1), (-1.0, -0.5, 0.0, 0.5, 1.0, 1.5)),
    ([(3, 4, 5)], 8, CUBE8, (3, 4, 5, 3, 4, 5, 1), CUBE8),
    ([(0, 0, 0)], 2, CUBE8, (0, 0, 0, 0, 0, 0, 1), (-2.0, -2.0, -2.0, -0.5, -0.5, -0.5)),
    ([(7, 7, 7)], 2, CUBE8, (7, 7, 7, 7, 7, 7, 1), (0.5, 0.5, 0.5, 2.0, 2.0, 2.0)),
    ([(0, 0, 0), (7, 7, 7)], 0, CUBE8, (0, 0, 0, 7, 7, 7, 1), CUBE8),
    ([(1, 6, 2), (5, 2, 3)], 0, CUBE8, (1, 2, 2, 5, 6, 3, 1), (-1.5, -1.0, -1.0, 1.0, 1.5, 0.0)),
    ([(1, 6, 2), (5, 2, 3)], 0, (-1.25, -3.0, -0.75, 0.75, 3.0, 9.0), (1, 2, 2, 5, 6, 3, 1), (-1.25, -1.0, -0.75, 0.75, 1.5, 0.0)),      # an outer box that cuts
    ([(1, 6, 2), (5, 2, 3)], 0, (1.0, -3.0, -3.0, 3.0, 3.0, 3.0), (1, 2, 2, 5, 6, 3, 2), (1.0, -3.0, -3.0, 3.0, 3.0, 3.0)),             # ... touches in x: lo == hi
    ([(1, 6, 2), (5, 2, 3)], 1, (5.0, 5.0, 5.0, 6.0, 6.0, 6.0), (1, 2, 2, 5, 6, 3, 2), (5.0, 5.0, 5.0, 6.0, 6.0, 6.0)),                  # ... disjoint
]


@pytest.mark.parametrize("case", range(len(TABLE)))
def test_the_restatement_gives_the_boxes_its_table_says(case):
    occupied, margin, outer, want_cells, want_box = TABLE[case]
    cells, box = F.voxel_box_ref(F.grid_with(G8, occupied), BMIN8, H8, 0.0, margin, outer)
    assert cells.dtype == torch.int32 and box.dtype == torch.float32
    assert tuple(cells.tolist()) == want_cells + (0,) and tuple(box.tolist()) == tuple(want_box)


def test_the_restatement_compares_as_the_select_does():
    nan, inf = float("nan"), float("inf")
    grid = lambda v: F.grid_with(4, [(1, 2, 3, v)], below=-inf)
    for thresh in (-0.5, 0.0, 0.5):
        status = lambda v: int(F.voxel_box_ref(grid(v), -1.0, 0.5, thresh, 0, (-1.0,) * 3 + (1.0,) * 3)[0][6])
        assert [status(v) for v in (thresh, nan, -inf, inf, thresh + 1e-3, thresh - 1e-3)] == [0, 0, 0, 1, 1, 0]
    # a grid of NaN, and one at the threshold everywhere, hold no occupied cell; one of +inf is all occupied
    for fill, want in ((nan, 0), (0.0, 0), (inf, 1)):
        cells, _ = F.voxel_box_ref(torch.full((4, 4, 4), fill), -1.0, 0.5, 0.0, 0, (-1.0,) * 3 + (1.0,) * 3)
        assert int(cells[6]) == want and (want == 0 or cells.tolist()[:6] == [0, 0, 0, 3, 3, 3])
    # a bound that is no fp32 number is rounded twice, as the kernel's: the product, then the sum
    h = F.cell_edge(7, -3.5, 3.5)
    _, box = F.voxel_box_ref(F.grid_with(7, [(2, 3, 4)]), -3.5, h, 0.0, 0, (-3.5,) * 3 + (3.5,) * 3)
    assert box.tolist() == list(F.box_of_cells((2, 3, 4), (2, 3, 4), -3.5, h))
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    assert float(box[3]) == float(f(-3.5) + f(3.0) * f(h)) and float(box[0]) == float(f(-3.5) + f(2.0) * f(h))


def test_the_grids_of_the_gpu_tests_are_no_degenerate_case():
    for G in (5, 64, 65):
        vox = F.random_fill(G, 0.01, G)
        share = float((vox > 0).float().mean())
        assert (0.002 < share < 0.03) if G > 5 else share < 0.1
    assert F.corners(5)[0] == (0, 0, 0) and F.corners(5)[-1] == (4, 4, 4) and len(set(F.corners(5))) == 8
    assert int((F.blob(16, (5, 6, 7), (9, 9, 8)) > 0).sum()) == 5 * 4 * 2
