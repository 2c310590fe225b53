"""The distortion loss (sys_param key "dist_weight"): what needs no GPU.

  the key          a finite float >= 0 (an int counts); a bool, a string, a negative, NaN or an infinity is a ValueError naming it;
                   absent or 0.0 the models and the loss are today's and carry no new state-dict key;
  RenderCall       `want_dist` sits between `prune` and `want_fg`, default False;
  refusals         a CPU model refuses a distortion-mode render / step with McnerfError; the regulariser entry points refuse host
                   tensors before the library is opened and, ahead of any device work, bad sizes, null pointers, d_dist without
                   moments and a non-finite depth scale;
  the header       include/mcnerf_reg.h parses with the core header's parser, its names disjoint from both other headers; one build()
                   call makes three libraries, each exporting exactly its own header;
  the references   tests/distortion_ref.py on every variant: non-decreasing rows, prefix form = O(S^2) definition to 1e-12, no interval
                   term for the far sample; the liveness conditions of family "b"; the identically-zero S = 2 rows.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import composite_ref as R
import distortion_ref as D
import mask_ref as M
from conftest import make_sys_param

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD = "mcnerf_reg_distortion_fwd", "mcnerf_reg_composite_bwd_w"


def _cfg():
    from oracle import mcnerf_oracle as O
    return O.RenderCfg(samples=16, scale=2, coarse=O.NetCfg(2, 32, (1,)), fine=O.NetCfg(2, 32, (1,)))


# ------------------------------------------------------------------------------------------------------------------ the key
@pytest.mark.parametrize("bad", [True, False, "1", None, -0.5, float("nan"), float("inf"), [1.0]])
def test_dist_weight_must_be_a_finite_float(bad):
    from mc_nerf_amd.model import MC_NeRF_Loss, NeRF_Model
    from mc_nerf_amd.model.loss import dist_weight_setting
    with pytest.raises(ValueError, match="dist_weight"):
        dist_weight_setting({"dist_weight": bad})
    with pytest.raises(ValueError, match="dist_weight"):
        NeRF_Model(make_sys_param(_cfg(), dist_weight=bad))
    with pytest.raises(ValueError, match="dist_weight"):
        MC_NeRF_Loss(make_sys_param(_cfg(), dist_weight=bad, data_img_h=8, data_img_w=8))


def test_dist_weight_default_and_values():
    from mc_nerf_amd.model import NeRF_Model
    from mc_nerf_amd.model.loss import dist_weight_setting
    assert dist_weight_setting({}) == 0.0 and dist_weight_setting({"dist_weight": 0}) == 0.0
    assert dist_weight_setting({"dist_weight": 1}) == 1.0 and dist_weight_setting({"dist_weight": 0.25}) == 0.25
    off, on = NeRF_Model(make_sys_param(_cfg())), NeRF_Model(make_sys_param(_cfg(), dist_weight=0.5))
    assert off.dist_weight == 0.0 and on.dist_weight == 0.5 and off.last_distortion is None and on.last_distortion is None
    assert off.mask_weight == 0.0 and on.mask_weight == 0.0
    assert list(off.state_dict()) == list(on.state_dict())            # no new parameter, no new buffer


def test_render_call_fields():
    from mc_nerf_amd.model.render import RenderCall
    call = RenderCall(*range(12))
    assert call.want_dist is False and call.want_fg is False and call.prune == 11
    assert RenderCall._fields[-3:] == ("prune", "want_dist", "want_fg")
    assert RenderCall(*range(12), want_dist=True).want_fg is False


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_a_cpu_model_refuses_distortion_mode():
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import NeRF_Model
    m = NeRF_Model(make_sys_param(_cfg(), dist_weight=0.5, data_img_h=8, data_img_w=8))
    d = torch.nn.functional.normalize(torch.randn(4, 3), dim=-1)
    with pytest.raises(McnerfError, match="dist_weight"):
        m.render_rays_train(d, -3.0 * d, 0, 1.0)


def test_a_cpu_mc_model_refuses_a_distortion_step():
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import MC_Model
    sp = S.make_sys_param("cpu", samples=8, scale=2, batch=16, H=8, W=8, coarse=(2, 32, [1]), fine=(2, 32, [1]), dist_weight=0.5)
    model = MC_Model(sp)
    S.init_cameras_near_gt(model)
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    with pytest.raises(McnerfError, match="dist_weight"):
        model((torch.rand(1, 64, 3), torch.tensor([0]), wpts, pts, wpts, pts), 20, "GLOBAL_OPTIM_EPOCH", 0.6)


def test_the_loss_term_is_the_weighted_sum_of_means():
    from mc_nerf_amd.model import MC_NeRF_Loss
    loss = MC_NeRF_Loss(make_sys_param(_cfg(), dist_weight=0.25, data_img_h=8, data_img_w=8))
    g = torch.Generator().manual_seed(1)
    c, f = torch.rand(7, generator=g).requires_grad_(True), torch.rand(7, generator=g).requires_grad_(True)
    v = loss.get_distortion_loss([c, f])
    assert float(v.detach()) == pytest.approx(0.25 * (float(c.detach().mean()) + float(f.detach().mean())), rel=1e-6)
    v.backward()
    assert torch.allclose(c.grad, torch.full((7,), 0.25 / 7)) and torch.allclose(f.grad, torch.full((7,), 0.25 / 7))
    assert float(loss.get_distortion_loss([c, None], weight=2.0).detach()) == pytest.approx(2.0 * float(c.detach().mean()), rel=1e-6)
    assert float(loss.get_distortion_loss([torch.zeros(0), None])) == 0.0
    with pytest.raises(ValueError, match="dist_weight"):
        loss.get_distortion_loss([c, f], weight=-1.0)
    with pytest.raises(ValueError, match="dist_weight"):
        loss.get_distortion_loss([c, f], weight=float("nan"))


def test_regulariser_ops_refuse_host_tensors_before_the_library_is_opened(monkeypatch):
    from mc_nerf_amd import _reg, ops
    from mc_nerf_amd._lib import McnerfError
    monkeypatch.setattr(_reg, "lib", lambda: pytest.fail("the library was opened"))
    sig, z, eps = torch.zeros(2, 3, 4), torch.linspace(1, 2, 3), torch.zeros(2, 3)
    with pytest.raises(McnerfError, match=FWD + r": sig_rgb .*no CPU fallback"):
        ops.distortion_fwd(sig, z, None, eps, 1.0, 8.0)
    with pytest.raises(McnerfError, match=BWD + r": sig_rgb .*no CPU fallback"):
        ops.composite_bwd_w(sig, z, None, eps, torch.zeros(2, 3), None, torch.zeros(2), torch.zeros(2, 16, dtype=torch.uint8), 1.0, 8.0)
    with pytest.raises(McnerfError, match="moments"):
        ops.composite_bwd_w(sig, z, None, eps, torch.zeros(2, 3), None, torch.zeros(2), None, 1.0, 8.0)
    with pytest.raises(McnerfError, match="z_rows"):
        ops.distortion_fwd(sig, None, None, eps, 1.0, 8.0, z_rows=torch.zeros(3, 3))


def test_entry_points_refuse_before_any_device_work():
    """Raw addresses that are never dereferenced: every refusal below is decided on the host (no GPU is needed)."""
    from mc_nerf_amd import _reg
    from mc_nerf_amd._lib import McnerfError
    P = 4096                                # a non-null "pointer"
    inf, nan = float("inf"), float("nan")
    # N = 0: no-ops, null pointers allowed
    _reg.call(FWD, None, None, 0, None, None, 0, 8, 1.0, 0.125, None, None, 0)
    _reg.call(BWD, None, None, 0, None, None, None, None, None, None, 1.0, 0.125, 0, 8, 1, None, None, 0)
    bad = [
        (FWD, (None, P, 0, None, P, 2, 8, 1.0, 0.125, P, P, 0)),                            # null sig_rgb
        (FWD, (P, None, 0, None, P, 2, 8, 1.0, 0.125, P, P, 0)),                            # null zgrid
        (FWD, (P, P, 0, None, None, 2, 8, 1.0, 0.125, P, P, 0)),                            # null eps
        (FWD, (P, P, 0, None, P, 2, 8, 1.0, 0.125, None, P, 0)),                            # null dist
        (FWD, (P, P, 0, None, P, 2, 8, 1.0, 0.125, P, None, 0)),                            # null moments
        (FWD, (P, P, 0, None, P, 2, 0, 1.0, 0.125, P, P, 0)),                               # S = 0
        (FWD, (P, P, 3, None, P, 2, 8, 1.0, 0.125, P, P, 0)),                               # z_stride neither 0 nor S
        (FWD, (P, P, 0, None, P, -1, 8, 1.0, 0.125, P, P, 0)),                              # N < 0
        (FWD, (P, P, 0, None, P, 1 << 21, 1 << 10, 1.0, 0.125, P, P, 0)),                   # N S >= 2^31
        (FWD, (P, P, 0, None, P, 2, 8, 1.0, inf, P, P, 0)),                                 # non-finite z_scale
        (FWD, (P, P, 0, None, P, 2, 8, 1.0, nan, P, P, 0)),
        (FWD, (P, P, 0, None, P, 0, 8, 1.0, nan, None, None, 0)),                           # ... even with no rays
        (BWD, (P, P, 0, None, P, P, None, P, P, 1.0, 0.125, 2, 2049, 1, P, None, 0)),       # S over the LDS bound
        (BWD, (None, P, 0, None, P, P, None, P, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),       # null sig_rgb
        (BWD, (P, None, 0, None, P, P, None, P, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),       # null zgrid
        (BWD, (P, P, 0, None, None, P, None, P, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),       # null eps
        (BWD, (P, P, 0, None, P, None, None, P, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),       # null d_rgb
        (BWD, (P, P, 0, None, P, P, None, P, P, 1.0, 0.125, 2, 8, 1, None, None, 0)),       # null output
        (BWD, (P, P, 5, None, P, P, None, P, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),          # z_stride neither 0 nor S
        (BWD, (P, P, 0, None, P, P, None, P, P, 1.0, 0.125, 1 << 21, 1 << 10, 1, P, None, 0)),   # N S >= 2^31
        (BWD, (P, P, 0, None, P, P, None, P, None, 1.0, 0.125, 2, 8, 1, P, None, 0)),       # d_dist without moments
        (BWD, (P, P, 0, None, P, P, None, None, P, 1.0, 0.125, 2, 8, 1, P, None, 0)),       # moments without d_dist
        (BWD, (P, P, 0, None, P, P, P, None, None, 1.0, inf, 2, 8, 1, P, None, 0)),         # non-finite z_scale
        (BWD, (P, P, 0, None, P, P, None, P, P, 1.0, nan, 2, 8, 1, P, None, 0)),
        (BWD, (P, P, 0, None, P, P, None, P, P, 1.0, 0.125, -1, 8, 1, P, None, 0)),         # N < 0
    ]
    for name, args in bad:
        with pytest.raises(McnerfError, match=name + r" failed \(-1\): " + name + ": invalid argument"):
            _reg.call(name, *args)


# ------------------------------------------------------------------------------------------------------------------ header / library
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(mcnerf_[a-z_0-9]+)\s*\(", text))


def test_the_regulariser_header_parses_and_its_names_are_its_own():
    from ctypes import c_float, c_int, c_void_p
    from mc_nerf_amd import _ext, _lib, _reg
    with open(os.path.join(ROOT, "include", "mcnerf_reg.h")) as f:
        params, defines = _lib.parse_header(f.read())
    assert params == _reg.PARAMS and defines == _reg.DEFINES
    assert sorted(_reg.SIGNATURES) == sorted(_declared("mcnerf_reg.h")) and len(_reg.SIGNATURES) == 4
    assert all(n.startswith("mcnerf_reg_") for n in _reg.SIGNATURES) and all(k.startswith("MCNERF_REG_") for k in _reg.DEFINES)
    assert _reg.ABI_VERSION == 1 and _reg.DEFINES["MCNERF_REG_MOMENT_BYTES"] == 16 and _reg.DEFINES["MCNERF_REG_BWD_MAX_SAMPLES"] == 2048
    assert not set(_reg.SIGNATURES) & set(_lib.SIGNATURES) and not set(_reg.SIGNATURES) & set(_ext.SIGNATURES)
    assert not set(_reg.DEFINES) & set(_lib.DEFINES) and not set(_reg.DEFINES) & set(_ext.DEFINES)
    at = {p[0]: (p[2], p[3]) for p in _reg.PARAMS[BWD][1]}
    assert at["moments"] == (c_void_p, torch.uint8) and at["d_dist"] == (c_void_p, torch.float32) and at["gmax_bits"] == (c_void_p, torch.int32)
    assert at["z_near"] == (c_float, None) and at["z_scale"] == (c_float, None) and at["N"] == (c_int, None)
    assert _reg.SIGNATURES[FWD][1][5:9] == [c_int, c_int, c_float, c_float]
    assert _reg.McnerfError is _lib.McnerfError and _reg.call is not _lib.call and _reg.call is not _ext.call
    # the extension binding keeps every attribute it has
    for name in ("LIB_PATH", "PARAMS", "DEFINES", "SIGNATURES", "ABI_VERSION", "lib", "loaded", "call", "McnerfError"):
        assert hasattr(_ext, name) and hasattr(_reg, name), name
    assert len(_ext.SIGNATURES) == 6 and _ext.ABI_VERSION == 1


def test_the_library_path_can_be_overridden():
    env = dict(os.environ, MCNREG_LIB="/nonexistent/libmcnreg.so", PYTHONPATH=ROOT)
    code = ("from mc_nerf_amd import _reg\n"
            "assert _reg.LIB_PATH == '/nonexistent/libmcnreg.so' and not _reg.loaded()\n"
            "try:\n    _reg.call('mcnerf_reg_distortion_fwd', None, None, 0, None, None, 0, 8, 1.0, 0.125, None, None, 0)\n"
            "except _reg.McnerfError as e:\n    assert 'not found' in str(e) and 'no CPU fallback' in str(e)\n"
            "else:\n    raise SystemExit('a missing library did not raise')\n")
    import sys
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)


@pytest.fixture(scope="module")
def built():
    from mc_nerf_amd import build
    if not os.path.isfile(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    core = build.build(verbose=False)
    return core, build.EXT_OUT, build.REG_OUT


def test_one_build_call_makes_three_libraries(built):
    from mc_nerf_amd import _reg, build
    core, ext, reg = built
    assert core == build.OUT and all(os.path.isfile(p) for p in built) and os.path.basename(reg) == "libmcnreg.so"
    assert build.REG_SOURCES == ["reg_api.hip", "distortion.hip"] and "mcnerf_distortion.h" in build.REG_HEADERS
    assert build.EXT_SOURCES == ["ext_api.hip", "mask.hip"]
    assert not set(build.REG_SOURCES) & (set(build.SOURCES) | set(build.EXT_SOURCES))
    assert all(os.path.isfile(os.path.join(build.CSRC, s)) for s in build.REG_SOURCES + build.REG_HEADERS)
    assert not any(f.startswith("-D") for f in build.FLAGS)
    l = _reg.lib()
    assert l.mcnerf_reg_abi_version() == _reg.ABI_VERSION and l.mcnerf_reg_last_error() is not None


def _exports(lib):
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_each_of_the_three_libraries_exports_its_own_header(built):
    core, ext, reg = built
    for lib, header in ((core, "mcnerf.h"), (ext, "mcnerf_ext.h"), (reg, "mcnerf_reg.h")):
        assert {s for s in _exports(lib) if s.startswith("mcnerf_")} == _declared(header), header
    assert not _declared("mcnerf_reg.h") & (_declared("mcnerf.h") | _declared("mcnerf_ext.h"))


def test_the_new_sources_have_no_preprocessor_conditionals():
    from mc_nerf_amd import build
    for name in build.REG_SOURCES + ["mcnerf_distortion.h"]:
        text = open(os.path.join(build.CSRC, name)).read()
        assert not re.findall(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", text, flags=re.M), name
    assert "#pragma once" in open(os.path.join(build.CSRC, "mcnerf_distortion.h")).read()


# ------------------------------------------------------------------------------------------------------------------ the references
VARIANTS = [(shape, family, rows) for shape in M.SHAPES for family in ("a", "b") for rows in (False, True)]


@pytest.mark.parametrize("shape, family, rows", VARIANTS)
def test_rows_prefix_form_and_far_sample(shape, family, rows):
    inp = D.variant(shape, family, rows, True)
    w, s, z = D.weights64(inp)
    N, S = w.shape
    assert bool((z[:, 1:] >= z[:, :-1]).all())                                # non-decreasing: what the O(S) form requires
    prefix = D.dist_prefix(w, s)
    for lo, hi in D._chunks(N, S, False):
        e = float((D.dist_pairs(w[lo:hi], s[lo:hi]) - prefix[lo:hi]).abs().max())
        assert e <= 1e-12, (shape, family, rows, lo, e)
    # the far sample has no interval term: its sentinel "interval" does not enter, whatever it is
    assert torch.equal(D.interval_term(w, s), D.interval_term(w, s, last=torch.zeros(N, dtype=torch.float64)))
    with_sentinel = D.interval_term(w, s, last=torch.full((N,), 1e10 * D.Z_SCALE, dtype=torch.float64))
    assert bool((with_sentinel[w[:, -1] > 1e-3] > 100.0).all())              # (it would dominate wherever the far sample has weight)
    assert bool((prefix <= (4.0 / 3.0) * w.sum(dim=1) ** 2 * (s[:, -1] - s[:, 0]) + 1e-12).all())      # the span bounds the term
    assert torch.equal(D.reference(D._slice(inp, 0, min(N, 8)), prefix=True)["dist"], prefix[:min(N, 8)])
    if D.is_identically_zero(shape, rows):
        assert bool((s[:, 1] == s[:, 0]).all())                               # the duplicated depth
        ref = D.reference(inp)
        assert float(ref["dist"].abs().max()) == 0.0 and float(ref["d_alone"].abs().max()) == 0.0


@pytest.mark.parametrize("rows", [False, True])
def test_family_b_is_live(rows):
    shares, grads = {}, {}
    for shape in M.SHAPES:
        inp = D.variant(shape, "b", rows, True)
        N, S = inp["sig_rgb"].shape[:2]
        if N == 53 and S >= 3:
            ref = D.reference(inp, prefix=S > 129)                            # (liveness only: the form is held to the definition above)
            shares[shape], grads[shape] = D.live_share(ref["dist"]), float(ref["d_alone"].abs().max())
    print("share of rays with dist > 1e-2:", {k: round(v, 2) for k, v in shares.items()}, " max|d_alone|:", {k: f"{v:.1e}" for k, v in grads.items()})
    assert len(shares) == 6 and min(shares.values()) >= D.LIVE_SHARE, shares
    assert min(grads.values()) > D.LIVE_GRAD, grads


def test_d_dist_is_drawn_per_ray_and_the_variant_is_mask_refs():
    a, m = D.variant("edge_S65", "b", True, False), M.variant("edge_S65", "b", True, False)
    assert a["d_dist"].shape == (53,) and torch.equal(a["d_dist"], D.variant("edge_S65", "b", True, True)["d_dist"])
    for k in m:
        assert (torch.equal(a[k], m[k]) if isinstance(m[k], torch.Tensor) else a[k] == m[k]), k
    assert "\0mask_ref" not in R.CASES and D.NEAR == 1.0 and D.FAR == 8.0 and abs(D.Z_SCALE - 1.0 / 7.0) < 1e-8


@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("shape", ["edge_S3", "edge_S65", "edge_S129", "one_ray"])
def test_fp32_restatement_against_fp64(shape, family):
    """The fp32 restatement (whose error sets the kernels' bar) is itself an fp32-grade statement of the fp64 one."""
    inp = D.variant(shape, family, True, False)
    ref, got = D.reference(inp), D.restated32(inp)
    for k in ("dist", "d_full", "d_alone"):
        e, _ = R.worst(got[k], ref[k])
        assert e <= 1e-5 * max(1.0, float(ref[k].abs().max())), (shape, family, k, e)
