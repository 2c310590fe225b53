"""Depth supervision (sys_param key "depth_weight"): what needs no GPU.

  the key          a finite float >= 0 (an int counts); a bool, a string, a negative, NaN or an infinity is a ValueError naming it;
                   absent or 0.0 the models and the loss are today's and carry no new state-dict key; RenderCall keeps its 14 fields,
                   the switch is RenderSettings.want_zexp (the last field, default False);
  refusals         a CPU model refuses a depth-mode render / step with McnerfError; the geometry entry points refuse host tensors
                   before the library is opened and, ahead of any device work, bad sizes, null pointers, bad segment tables, d_dist
                   without moments, a non-finite depth scale where it is read, a negative or non-finite weight;
  the header       include/mcnerf_geo.h parses with the core header's parser, its names disjoint from the three other headers; one
                   build() call makes four libraries, each exporting exactly its own header; the source lists are disjoint; no
                   preprocessor conditionals in the new sources; with MCNGEO_LIB pointing nowhere the package imports and default-key
                   models are constructed without the library being opened;
  the references   tests/depth_ref.py on every variant: autograd d zexp / d alpha against the closed form to 1e-12; the
                   semi-transparent share of the variants used; the fp32 restatement against fp64; the loss's n_valid = 0 branch;
  host helpers     z_depth_to_ray_distance on a pinhole camera (ray distance * cos theta = z); blob_scene_depth is 0 exactly where
                   alpha < 0.5; DeviceImageSet(depth=...) asserts shape and dtype.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import composite_ref as R
import depth_ref as Z
import mask_ref as M
from conftest import make_sys_param

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD, GATHER, LOSS = "mcnerf_geo_depth_fwd", "mcnerf_geo_composite_bwd_z", "mcnerf_geo_gather_depth", "mcnerf_geo_depth_loss"


def _cfg():
    from oracle import mcnerf_oracle as O
    return O.RenderCfg(samples=16, scale=2, coarse=O.NetCfg(2, 32, (1,)), fine=O.NetCfg(2, 32, (1,)))


# ------------------------------------------------------------------------------------------------------------------ the key
@pytest.mark.parametrize("bad", [True, False, "1", None, -0.5, float("nan"), float("inf"), -float("inf"), [1.0]])
def test_depth_weight_must_be_a_finite_float(bad):
    from mc_nerf_amd.model import MC_NeRF_Loss, NeRF_Model
    from mc_nerf_amd.model.loss import depth_weight_setting
    with pytest.raises(ValueError, match="depth_weight"):
        depth_weight_setting({"depth_weight": bad})
    with pytest.raises(ValueError, match="depth_weight"):
        NeRF_Model(make_sys_param(_cfg(), depth_weight=bad))
    with pytest.raises(ValueError, match="depth_weight"):
        MC_NeRF_Loss(make_sys_param(_cfg(), depth_weight=bad, data_img_h=8, data_img_w=8))


def test_depth_weight_default_and_values():
    from mc_nerf_amd.model import MC_NeRF_Loss, NeRF_Model
    from mc_nerf_amd.model.loss import depth_weight_setting
    assert depth_weight_setting({}) == 0.0 and depth_weight_setting({"depth_weight": 0}) == 0.0
    assert depth_weight_setting({"depth_weight": 1}) == 1.0 and depth_weight_setting({"depth_weight": 0.25}) == 0.25
    off, zero, on = NeRF_Model(make_sys_param(_cfg())), NeRF_Model(make_sys_param(_cfg(), depth_weight=0.0)), NeRF_Model(make_sys_param(_cfg(), depth_weight=0.5))
    assert off.depth_weight == 0.0 and zero.depth_weight == 0.0 and on.depth_weight == 0.5
    assert off.settings.want_zexp is False and zero.settings.want_zexp is False and on.settings.want_zexp is True
    assert off.last_expected_depth is None and on.last_expected_depth is None
    assert on.mask_weight == 0.0 and on.dist_weight == 0.0
    assert list(off.state_dict()) == list(on.state_dict())            # no new parameter, no new buffer
    assert MC_NeRF_Loss(make_sys_param(_cfg(), depth_weight=2, data_img_h=8, data_img_w=8)).depth_weight == 2.0


def test_the_switch_rides_on_render_settings():
    import dataclasses
    from mc_nerf_amd.model.render import RenderCall, RenderSettings
    assert len(RenderCall._fields) == 14 and RenderCall._fields[-1] == "want_fg" and "want_zexp" not in RenderCall._fields
    fields = [f.name for f in dataclasses.fields(RenderSettings)]
    assert fields[-1] == "want_zexp" and RenderSettings(16, 2, 0.1, 0.0, True).want_zexp is False


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_a_cpu_model_refuses_depth_mode():
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import NeRF_Model
    m = NeRF_Model(make_sys_param(_cfg(), depth_weight=0.5, data_img_h=8, data_img_w=8))
    d = torch.nn.functional.normalize(torch.randn(4, 3), dim=-1)
    with pytest.raises(McnerfError, match="depth_weight"):
        m.render_rays_train(d, -3.0 * d, 0, 1.0)


def test_a_cpu_mc_model_refuses_a_depth_step():
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import MC_Model
    sp = S.make_sys_param("cpu", samples=8, scale=2, batch=16, H=8, W=8, coarse=(2, 32, [1]), fine=(2, 32, [1]), depth_weight=0.5)
    model = MC_Model(sp)
    S.init_cameras_near_gt(model)
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    with pytest.raises(McnerfError, match="depth_weight"):
        model((torch.rand(1, 64, 3), torch.tensor([0]), wpts, pts, wpts, pts), 20, "GLOBAL_OPTIM_EPOCH", 0.6)


def test_get_depth_loss_refuses_a_bad_weight():
    from mc_nerf_amd.model import MC_NeRF_Loss
    loss = MC_NeRF_Loss(make_sys_param(_cfg(), depth_weight=0.25, data_img_h=8, data_img_w=8))
    z = torch.rand(7)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="depth_weight"):
            loss.get_depth_loss([z, z, z], 1.0, 8.0, weight=bad)


def test_geometry_ops_refuse_host_tensors_before_the_library_is_opened(monkeypatch):
    from mc_nerf_amd import _geo, ops
    from mc_nerf_amd._lib import McnerfError
    monkeypatch.setattr(_geo, "lib", lambda: pytest.fail("the library was opened"))
    sig, z, eps = torch.zeros(2, 3, 4), torch.linspace(1, 2, 3), torch.zeros(2, 3)
    with pytest.raises(McnerfError, match=FWD + r": sig_rgb .*no CPU fallback"):
        ops.expected_depth(sig, z, None, eps)
    with pytest.raises(McnerfError, match=BWD + r": sig_rgb .*no CPU fallback"):
        ops.composite_bwd_z(sig, z, None, eps, torch.zeros(2, 3), None, None, None, torch.zeros(2), 1.0, 8.0)
    with pytest.raises(McnerfError, match="moments"):
        ops.composite_bwd_z(sig, z, None, eps, torch.zeros(2, 3), None, torch.zeros(2), None, torch.zeros(2), 1.0, 8.0)
    with pytest.raises(McnerfError, match="d_zexp"):
        ops.composite_bwd_z(sig, z, None, eps, torch.zeros(2, 3), None, None, None, torch.zeros(3), 1.0, 8.0)
    with pytest.raises(McnerfError, match="z_rows"):
        ops.expected_depth(sig, None, None, eps, z_rows=torch.zeros(3, 3))
    with pytest.raises(McnerfError, match=GATHER + r": depth .*no CPU fallback"):
        ops.gather_depth(torch.ones(2, 6), [0], [0, 4], torch.zeros(4, dtype=torch.int64))
    with pytest.raises(McnerfError, match=r"\[C, H\*W\]"):
        ops.gather_depth(torch.ones(2, 3, 2), [0], [0, 4], torch.zeros(4, dtype=torch.int64))
    with pytest.raises(McnerfError, match=LOSS + r": zexp_c .*no CPU fallback"):
        ops.depth_loss(torch.ones(4), None, torch.ones(4), 1.0, 8.0, 0.5)
    with pytest.raises(McnerfError, match="same 4 rays"):
        ops.depth_loss(torch.ones(4), None, torch.ones(5), 1.0, 8.0, 0.5)


def test_entry_points_refuse_before_any_device_work():
    """Raw addresses that are never dereferenced: every refusal below is decided on the host (no GPU is needed)."""
    import ctypes
    from mc_nerf_amd import _geo
    from mc_nerf_amd._lib import McnerfError
    P = 4096                                # a non-null "pointer"
    inf, nan = float("inf"), float("nan")
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)
    # N = 0 / n = 0: no-ops, null pointers allowed
    _geo.call(FWD, None, None, 0, None, None, 0, 8, None, 0)
    _geo.call(BWD, None, None, 0, None, None, None, None, None, None, None, nan, nan, 0, 8, 1, None, None, 0)      # (no d_dist: the span is not read)
    _geo.call(GATHER, None, 1, 10, arr([0]), arr([0, 0]), 1, None, 0, None, 0)
    _geo.call(LOSS, None, None, None, 0, 1.0, 0.125, 0.5, None, None, None, 0)
    bad = [
        (FWD, (None, P, 0, None, P, 2, 8, P, 0)),                                            # null sig_rgb
        (FWD, (P, None, 0, None, P, 2, 8, P, 0)),                                            # null zgrid
        (FWD, (P, P, 0, None, None, 2, 8, P, 0)),                                            # null eps
        (FWD, (P, P, 0, None, P, 2, 8, None, 0)),                                            # null zexp
        (FWD, (P, P, 0, None, P, 2, 0, P, 0)),                                               # S = 0
        (FWD, (P, P, 3, None, P, 2, 8, P, 0)),                                               # z_stride neither 0 nor S
        (FWD, (P, P, 0, None, P, -1, 8, P, 0)),                                              # N < 0
        (FWD, (P, P, 0, None, P, 1 << 21, 1 << 10, P, 0)),                                   # N S >= 2^31
        (BWD, (P, P, 0, None, P, P, None, None, None, P, 1.0, 0.125, 2, 2049, 1, P, None, 0)),     # S over the LDS bound
        (BWD, (None, P, 0, None, P, P, None, None, None, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),     # null sig_rgb
        (BWD, (P, None, 0, None, P, P, None, None, None, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),     # null zgrid
        (BWD, (P, P, 0, None, None, P, None, None, None, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),     # null eps
        (BWD, (P, P, 0, None, P, None, None, None, None, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),     # null d_rgb
        (BWD, (P, P, 0, None, P, P, None, None, None, P, 1.0, 0.125, 2, 8, 1, None, None, 0)),     # null output
        (BWD, (P, P, 5, None, P, P, None, None, None, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),        # z_stride neither 0 nor S
        (BWD, (P, P, 0, None, P, P, None, None, None, P, 1.0, 0.125, 1 << 21, 1 << 10, 1, P, None, 0)),   # N S >= 2^31
        (BWD, (P, P, 0, None, P, P, None, P, None, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),           # d_dist without moments
        (BWD, (P, P, 0, None, P, P, None, None, P, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),           # moments without d_dist
        (BWD, (P, P, 0, None, P, P, None, P, P, P, 1.0, inf, 2, 8, 1, P, None, 0)),                # non-finite z_scale with d_dist
        (BWD, (P, P, 0, None, P, P, None, P, P, P, nan, 0.125, 2, 8, 1, P, None, 0)),              # non-finite z_near with d_dist
        (BWD, (P, P, 0, None, P, P, None, None, None, P, 1.0, 0.125, -1, 8, 1, P, None, 0)),       # N < 0
        (GATHER, (P, 3, 10, None, arr([0, 4]), 1, P, 4, P, 0)),                              # null table
        (GATHER, (P, 3, 10, arr([3]), arr([0, 4]), 1, P, 4, P, 0)),                          # camera outside [0, C)
        (GATHER, (P, 3, 10, arr([-1]), arr([0, 4]), 1, P, 4, P, 0)),
        (GATHER, (P, 3, 10, arr([0, 1]), arr([0, 6, 5]), 2, P, 5, P, 0)),                    # not monotone
        (GATHER, (P, 3, 10, arr([0]), arr([1, 4]), 1, P, 4, P, 0)),                          # does not start at 0
        (GATHER, (P, 3, 10, arr([0]), arr([0, 3]), 1, P, 4, P, 0)),                          # does not end at n
        (GATHER, (P, 3, 10, arr([0] * 65), arr(list(range(66))), 65, P, 65, P, 0)),          # K over the bound
        (GATHER, (P, 3, 10, arr([0]), arr([0, 4]), 0, P, 4, P, 0)),                          # K = 0
        (GATHER, (P, 3, 0, arr([0]), arr([0, 4]), 1, P, 4, P, 0)),                           # HW = 0
        (GATHER, (None, 3, 10, arr([0]), arr([0, 4]), 1, P, 4, P, 0)),                       # null depth
        (GATHER, (P, 3, 10, arr([0]), arr([0, 4]), 1, None, 4, P, 0)),                       # null pix
        (GATHER, (P, 3, 10, arr([0]), arr([0, 4]), 1, P, 4, None, 0)),                       # null out
        (LOSS, (P, None, P, -1, 1.0, 0.125, 0.5, P, P, None, 0)),                            # n < 0
        (LOSS, (P, None, P, 4, 1.0, 0.125, -0.5, P, P, None, 0)),                            # negative weight
        (LOSS, (P, None, P, 4, 1.0, 0.125, inf, P, P, None, 0)),                             # non-finite weight
        (LOSS, (P, None, P, 4, 1.0, 0.125, nan, P, P, None, 0)),
        (LOSS, (P, None, P, 4, nan, 0.125, 0.5, P, P, None, 0)),                             # non-finite z_near
        (LOSS, (P, None, P, 4, 1.0, inf, 0.5, P, P, None, 0)),                               # non-finite z_scale
        (LOSS, (P, None, P, 0, 1.0, inf, 0.5, P, P, None, 0)),                               # ... even with no rays
        (LOSS, (None, None, P, 4, 1.0, 0.125, 0.5, P, P, None, 0)),                          # null zexp_c
        (LOSS, (P, None, None, 4, 1.0, 0.125, 0.5, P, P, None, 0)),                          # null d_gt
        (LOSS, (P, None, P, 4, 1.0, 0.125, 0.5, None, P, None, 0)),                          # null out
        (LOSS, (P, None, P, 4, 1.0, 0.125, 0.5, P, None, None, 0)),                          # null d_c
        (LOSS, (P, P, P, 4, 1.0, 0.125, 0.5, P, P, None, 0)),                                # zexp_f without d_f
        (LOSS, (P, None, P, 4, 1.0, 0.125, 0.5, P, P, P, 0)),                                # d_f without zexp_f
    ]
    for name, args in bad:
        with pytest.raises(McnerfError, match=name + r" failed \(-1\): " + name + ": invalid argument"):
            _geo.call(name, *args)


# ------------------------------------------------------------------------------------------------------------------ header / library
HEADERS = ("mcnerf.h", "mcnerf_ext.h", "mcnerf_reg.h", "mcnerf_geo.h")


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(mcnerf_[a-z_0-9]+)\s*\(", text))


def test_the_geometry_header_parses_and_its_names_are_its_own():
    from ctypes import c_float, c_int, c_longlong, c_void_p
    from mc_nerf_amd import _ext, _geo, _lib, _reg
    with open(os.path.join(ROOT, "include", "mcnerf_geo.h")) as f:
        params, defines = _lib.parse_header(f.read())
    assert params == _geo.PARAMS and defines == _geo.DEFINES
    assert sorted(_geo.SIGNATURES) == sorted(_declared("mcnerf_geo.h")) and len(_geo.SIGNATURES) == 6
    assert all(n.startswith("mcnerf_geo_") for n in _geo.SIGNATURES) and all(k.startswith("MCNERF_GEO_") for k in _geo.DEFINES)
    assert _geo.ABI_VERSION == 1 and _geo.DEFINES["MCNERF_GEO_BWD_MAX_SAMPLES"] == 2048 and _geo.DEFINES["MCNERF_GEO_DEPTH_LOSS_OUT"] == 260
    for other in (_lib, _ext, _reg):
        assert not set(_geo.SIGNATURES) & set(other.SIGNATURES) and not set(_geo.DEFINES) & set(other.DEFINES)
    at = {p[0]: (p[2], p[3]) for p in _geo.PARAMS[BWD][1]}
    assert at["moments"] == (c_void_p, torch.uint8) and at["d_zexp"] == (c_void_p, torch.float32) and at["gmax_bits"] == (c_void_p, torch.int32)
    assert at["z_near"] == (c_float, None) and at["z_scale"] == (c_float, None) and at["N"] == (c_int, None)
    ag = {p[0]: (p[2], p[3]) for p in _geo.PARAMS[GATHER][1]}
    assert ag["HW"] == (c_longlong, None) and ag["seg_cam"] == (c_void_p, _lib.HOST) and ag["pix"] == (c_void_p, torch.int64)
    assert _geo.McnerfError is _lib.McnerfError and _geo.call not in (_lib.call, _ext.call, _reg.call)
    for name in ("LIB_PATH", "PARAMS", "DEFINES", "SIGNATURES", "ABI_VERSION", "lib", "loaded", "call", "McnerfError"):
        assert hasattr(_geo, name), name
    # the three pinned ABIs are what they were
    assert _lib.ABI_VERSION == 7 and len(_lib.SIGNATURES) == 53 and len(_ext.SIGNATURES) == 6 and len(_reg.SIGNATURES) == 4


def test_a_missing_library_is_never_opened_by_default_key_models():
    env = dict(os.environ, MCNGEO_LIB="/nonexistent/libmcngeo.so", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    code = ("import mc_nerf_amd\n"
            "from mc_nerf_amd import _geo, ops, synthetic as S\n"
            "from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, NeRF_Model\n"
            "assert _geo.LIB_PATH == '/nonexistent/libmcngeo.so' and not _geo.loaded()\n"
            "sp = S.make_sys_param('cpu', samples=8, scale=2, batch=16, H=8, W=8, coarse=(2, 32, [1]), fine=(2, 32, [1]))\n"
            "NeRF_Model(sp); MC_Model(sp); MC_NeRF_Loss(sp)\n"
            "NeRF_Model(dict(sp, depth_weight=0.0))\n"
            "assert not _geo.loaded()\n"
            "try:\n    _geo.call('mcnerf_geo_depth_fwd', None, None, 0, None, None, 0, 8, None, 0)\n"
            "except _geo.McnerfError as e:\n    assert 'not found' in str(e) and 'no CPU fallback' in str(e)\n"
            "else:\n    raise SystemExit('a missing library did not raise')\n")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)


@pytest.fixture(scope="module")
def built():
    from mc_nerf_amd import build
    if not os.path.isfile(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    core = build.build(verbose=False)
    return core, build.EXT_OUT, build.REG_OUT, build.GEO_OUT


def test_one_build_call_makes_four_libraries(built):
    from mc_nerf_amd import _geo, build
    core, ext, reg, geo = built
    assert core == build.OUT and all(os.path.isfile(p) for p in built) and os.path.basename(geo) == "libmcngeo.so"
    assert build.GEO_SOURCES == ["geo_api.hip", "depth.hip"] and "mcnerf_depth.h" in build.GEO_HEADERS
    assert "mcnerf_composite.h" in build.GEO_HEADERS and "mcnerf_wave.h" in build.GEO_HEADERS
    assert not set(build.GEO_SOURCES) & (set(build.SOURCES) | set(build.EXT_SOURCES) | set(build.REG_SOURCES))
    assert all(os.path.isfile(os.path.join(build.CSRC, s)) for s in build.GEO_SOURCES + build.GEO_HEADERS)
    assert not any(f.startswith("-D") for f in build.FLAGS) and not any(s in build.FILE_FLAGS for s in build.GEO_SOURCES)
    l = _geo.lib()
    assert l.mcnerf_geo_abi_version() == _geo.ABI_VERSION and l.mcnerf_geo_last_error() is not None


def _exports(lib):
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_each_of_the_four_libraries_exports_its_own_header(built):
    from mc_nerf_amd import _geo
    sets = []
    for lib, header in zip(built, HEADERS):
        sets.append({s for s in _exports(lib) if s.startswith("mcnerf_")})
        assert sets[-1] == _declared(header), header
    assert sets[3] == set(_geo.SIGNATURES)
    for i in range(4):
        for j in range(i + 1, 4):
            assert not sets[i] & sets[j], (HEADERS[i], HEADERS[j])


def test_the_new_sources_have_no_preprocessor_conditionals():
    from mc_nerf_amd import build
    for name in build.GEO_SOURCES + ["mcnerf_depth.h"]:
        text = open(os.path.join(build.CSRC, name)).read()
        assert not re.findall(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", text, flags=re.M), name
        assert "asm" not in re.sub(r"//.*", "", text), name
    assert "#pragma once" in open(os.path.join(build.CSRC, "mcnerf_depth.h")).read()


# ------------------------------------------------------------------------------------------------------------------ the references
VARIANTS = [(shape, family, rows) for shape in M.SHAPES for family in ("a", "b") for rows in (False, True)]


@pytest.mark.parametrize("shape, family, rows", VARIANTS)
def test_autograd_is_the_closed_form(shape, family, rows):
    """d zexp / d alpha_j = T_j z_j - sum_{k>j} w_k z_k / u_j, and 0 <= zexp <= the far depth (sum w <= 1 + 1e-10 S; it is below 1
    where the far sample is not opaque: the planted "last" ray)."""
    inp = Z.variant(shape, family, rows, True)
    auto, closed = Z.alpha_forms(inp)
    e, at = R.worst(auto, closed)
    assert e <= 1e-12, (shape, family, rows, e, at)
    zexp, z = Z.reference(Z.D._slice(inp, 0, min(53, inp["sig_rgb"].shape[0])))["zexp"], M._z32(inp).double()[:53]
    assert bool((zexp >= 0.0).all()) and bool((zexp <= z[:, -1] * (1 + 1e-6)).all())


@pytest.mark.parametrize("rows", [False, True])
def test_the_variants_used_have_semi_transparent_rays(rows):
    """The table's own random rays (family "a") all have a front weight of 0 or 1 (mask_ref) and would not exercise the term on their
    own: the parity runs use family "b" beside them.  Every "b" variant that redraws rays (N > 4) and has an interval of non-zero
    length (not the S = 2 rows: one duplicated depth) reports a non-zero semi-transparent share, at 53 rays and S >= 3 the share
    mask_ref names; and on EVERY variant, "a" ones included, the gradient of the term alone is not identically zero."""
    shares = {}
    for shape in M.SHAPES:
        for family in ("a", "b"):
            inp = Z.variant(shape, family, rows, True)
            _, fg = M.forward64(inp["sig_rgb"], M._z32(inp), inp["eps"], True)
            share = shares[shape, family] = M.semi_transparent_share(fg)
            N, S = inp["sig_rgb"].shape[:2]
            if family == "b" and N > 4 and not (S == 2 and rows):
                assert share > 0.0, (shape, share)
            if family == "b" and N == 53 and S >= 3:
                assert share >= M.FRACTION, (shape, share)
            if N <= 53:
                assert float(Z.reference(inp)["d_z"].abs().max()) > 0.0, (shape, family)
    print({f"{k[0]} {k[1]}": round(v, 3) for k, v in shares.items()})


def test_d_zexp_is_drawn_per_ray_and_the_variant_is_distortion_refs():
    a, d = Z.variant("edge_S65", "b", True, False), Z.D.variant("edge_S65", "b", True, False)
    assert a["d_zexp"].shape == (53,) and torch.equal(a["d_zexp"], Z.variant("edge_S65", "b", True, True)["d_zexp"])
    assert not torch.equal(a["d_zexp"], a["d_dist"]) and not torch.equal(a["d_zexp"], a["d_fg"])
    for k in d:
        assert (torch.equal(a[k], d[k]) if isinstance(d[k], torch.Tensor) else a[k] == d[k]), k
    assert "\0mask_ref" not in R.CASES and Z.NEAR == 1.0 and Z.FAR == 8.0 and set(Z.ALL_FOUR) <= set(M.SHAPES)


@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("shape", ["edge_S3", "edge_S65", "edge_S129", "one_ray"])
def test_fp32_restatement_against_fp64(shape, family):
    """The fp32 restatement (whose error sets the kernels' bar) is itself an fp32-grade statement of the fp64 one."""
    inp = Z.variant(shape, family, True, False)
    ref, got = Z.reference(inp, all_four=True), Z.restated32(inp, all_four=True)
    assert set(ref) == set(got) == {"zexp", "d_rz", "d_z", "d_all"}
    for k in ref:
        e, _ = R.worst(got[k], ref[k])
        assert e <= 1e-5 * max(1.0, float(ref[k].abs().max())), (shape, family, k, e)
    assert float(ref["d_z"].abs().max()) > 1e-3                                 # the term is live


def test_loss64_counts_only_measurements():
    g = torch.Generator().manual_seed(3)
    zc, zf = 1.0 + 7.0 * torch.rand(6, generator=g), 1.0 + 7.0 * torch.rand(6, generator=g)
    d = torch.tensor([2.0, 0.0, -1.0, float("nan"), float("inf"), 5.0])
    v, m, nv, d_c, d_f = Z.loss64(zc, zf, d, 1.0, 8.0, 0.5)
    want = (((zc[0] - 2.0) / 7.0) ** 2 + ((zc[5] - 5.0) / 7.0) ** 2 + ((zf[0] - 2.0) / 7.0) ** 2 + ((zf[5] - 5.0) / 7.0) ** 2).double() / 2.0
    assert nv == 2 and m == pytest.approx(float(want), rel=1e-6) and v == pytest.approx(0.5 * float(want), rel=1e-6)
    assert d_c[1:5].abs().max() == 0.0 and d_f[1:5].abs().max() == 0.0
    assert float(d_c[0]) == pytest.approx(2 * 0.5 / 7.0 / 2 * float(zc[0] - 2.0) / 7.0, rel=1e-6)
    v0, m0, nv0, d_c0, d_f0 = Z.loss64(zc, None, torch.tensor([0.0, -3.0, float("nan"), float("-inf"), 0.0, 0.0]), 1.0, 8.0, 0.5)
    assert (v0, m0, nv0) == (0.0, 0.0, 0) and d_f0 is None and float(d_c0.abs().max()) == 0.0 and bool(torch.isfinite(d_c0).all())


# ------------------------------------------------------------------------------------------------------------------ host helpers
def test_z_depth_to_ray_distance_on_a_pinhole_camera():
    from mc_nerf_amd.data import z_depth_to_ray_distance
    H, W = 5, 7
    K = torch.tensor([[9.0, 0.0, 3.3], [0.0, 8.0, 2.6], [0.0, 0.0, 1.0]])
    g = torch.Generator().manual_seed(1)
    z = 1.0 + 4.0 * torch.rand(H * W, generator=g)
    z[3], z[4], z[5], z[6] = 0.0, -1.0, float("nan"), float("inf")
    r = z_depth_to_ray_distance(z, K, H, W)
    assert r.shape == z.shape and r.dtype == z.dtype
    pid = torch.arange(H * W)
    u, v = (pid % W).double() + 0.5, (pid // W).double() + 0.5
    ray = torch.stack([(u - 3.3) / 9.0, (v - 2.6) / 8.0, torch.ones_like(u)], -1)
    cos = 1.0 / ray.norm(dim=-1)                                                # angle between the pixel's ray and the optical axis
    ok = torch.isfinite(z) & (z > 0)
    assert float((r.double() * cos - z.double())[ok].abs().max()) <= 1e-6       # ray distance * cos theta = z
    assert bool((r[ok] >= z[ok]).all()) and float(r[3]) == 0.0 and float(r[4]) < 0.0 and bool(torch.isnan(r[5])) and float(r[6]) == float("inf")
    # [C, H, W] with per-camera intrinsics
    Ks = torch.stack([K, K * torch.tensor([[2.0, 1.0, 1.0], [1.0, 2.0, 1.0], [1.0, 1.0, 1.0]])])
    r2 = z_depth_to_ray_distance(z.reshape(1, H, W).expand(2, H, W).contiguous(), Ks, H, W)
    assert r2.shape == (2, H, W) and torch.equal(torch.nan_to_num(r2[0].reshape(-1)), torch.nan_to_num(r))
    assert bool((r2[1].reshape(-1)[ok] <= r[ok]).all())                         # twice the focal length: narrower rays


def test_blob_scene_depth_is_zero_exactly_off_the_object():
    from mc_nerf_amd import synthetic as S
    g = torch.Generator().manual_seed(2)
    o = torch.nn.functional.normalize(torch.randn(400, 3, generator=g), dim=-1) * 3.0
    d = torch.nn.functional.normalize(-o + 0.9 * torch.randn(400, 3, generator=g), dim=-1)
    depth, alpha = S.blob_scene_depth(d, o, 1.0, 8.0, 384), S.blob_scene_alpha(d, o)
    assert depth.shape == (400,) and torch.equal(depth == 0.0, alpha < 0.5)
    hit = alpha >= 0.5
    assert 20 < int(hit.sum()) < 380                                            # both kinds of ray are there
    assert bool((depth[hit] > 1.0).all()) and bool((depth[hit] < 8.0).all())
    # the blob centres lie within 0.62 of the origin, three of their sigmas (<= 0.32) reach 1.6, and the cameras are 3 away
    assert bool((depth[hit] > 1.4).all()) and bool((depth[hit] < 4.6).all())


def test_device_image_set_checks_its_depth():
    from mc_nerf_amd.data import DeviceImageSet
    img = torch.zeros(2, 12, 4, dtype=torch.uint8)
    assert DeviceImageSet(img, 3, 4).depth is None
    s = DeviceImageSet(img, 3, 4, depth=torch.ones(2, 12))
    assert s.depth.shape == (2, 12) and s.depth.dtype == torch.float32 and s.depth.is_contiguous() and len(s) == 2
    for bad in (torch.ones(2, 11), torch.ones(3, 12), torch.ones(2, 3, 4), torch.ones(2, 12, dtype=torch.float64), torch.ones(2, 12, dtype=torch.float16)):
        with pytest.raises(AssertionError):
            DeviceImageSet(img, 3, 4, depth=bad)
