"""Alpha-mask supervision (sys_param key "mask_weight"): what needs no GPU.

  the key          a finite float >= 0 (an int counts); a bool, a string, a negative, NaN or an infinity is a ValueError naming it;
                   absent or 0.0 the models and the loss are today's and carry no new state-dict key;
  refusals         a CPU model refuses a mask-mode render / step with McnerfError; the extension entry points refuse host tensors and,
                   ahead of any device work, bad sizes, null pointers and bad segment tables;
  the header       include/mcnerf_ext.h parses with the core header's parser; the library builds in the same build() call, exports
                   exactly what the header declares, and libmcnerf.so still exports only the core ABI;
  the references   tests/mask_ref.py: the fp32 restatement against fp64, the far-plane fact (sum_j w_j = 1 on every ray, fg is what
                   varies) and the share of semi-transparent rays of family "b".
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import composite_ref as R
import mask_ref as M
from conftest import make_sys_param

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    from oracle import mcnerf_oracle as O
    return O.RenderCfg(samples=16, scale=2, coarse=O.NetCfg(2, 32, (1,)), fine=O.NetCfg(2, 32, (1,)))


# ------------------------------------------------------------------------------------------------------------------ the key
@pytest.mark.parametrize("bad", [True, False, "1", None, -0.5, float("nan"), float("inf"), [1.0]])
def test_mask_weight_must_be_a_finite_float(bad):
    from mc_nerf_amd.model import MC_NeRF_Loss, NeRF_Model
    from mc_nerf_amd.model.loss import mask_weight_setting
    with pytest.raises(ValueError, match="mask_weight"):
        mask_weight_setting({"mask_weight": bad})
    with pytest.raises(ValueError, match="mask_weight"):
        NeRF_Model(make_sys_param(_cfg(), mask_weight=bad))
    with pytest.raises(ValueError, match="mask_weight"):
        MC_NeRF_Loss(make_sys_param(_cfg(), mask_weight=bad, data_img_h=8, data_img_w=8))


def test_mask_weight_default_and_values():
    from mc_nerf_amd.model import NeRF_Model
    from mc_nerf_amd.model.loss import mask_weight_setting
    assert mask_weight_setting({}) == 0.0 and mask_weight_setting({"mask_weight": 0}) == 0.0
    assert mask_weight_setting({"mask_weight": 1}) == 1.0 and mask_weight_setting({"mask_weight": 0.25}) == 0.25
    off, on = NeRF_Model(make_sys_param(_cfg())), NeRF_Model(make_sys_param(_cfg(), mask_weight=0.5))
    assert off.mask_weight == 0.0 and on.mask_weight == 0.5 and off.last_front_weight is None and on.last_front_weight is None
    assert list(off.state_dict()) == list(on.state_dict())            # no new parameter, no new buffer


def test_render_call_default_is_off():
    from mc_nerf_amd.model.render import RenderCall
    call = RenderCall(*range(12))
    assert call.want_fg is False and call.prune == 11 and RenderCall._fields[-1] == "want_fg"


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_a_cpu_model_refuses_mask_mode():
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import MC_NeRF_Loss, NeRF_Model
    sp = make_sys_param(_cfg(), mask_weight=0.5, data_img_h=8, data_img_w=8)
    m = NeRF_Model(sp)
    d = torch.nn.functional.normalize(torch.randn(4, 3), dim=-1)
    with pytest.raises(McnerfError, match="mask_weight"):
        m.render_rays_train(d, -3.0 * d, 0, 1.0)
    with pytest.raises(McnerfError, match="no CPU fallback"):         # the loss of host tensors: refused before the library is opened
        MC_NeRF_Loss(sp).get_mask_loss([torch.rand(4), torch.rand(4), torch.rand(4)])
    with pytest.raises(ValueError, match="mask_weight"):
        MC_NeRF_Loss(sp).get_mask_loss([torch.rand(4), None, torch.rand(4)], weight=-1.0)


def test_a_cpu_mc_model_refuses_a_mask_step():
    from mc_nerf_amd import synthetic as S
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import MC_Model
    sp = S.make_sys_param("cpu", samples=8, scale=2, batch=16, H=8, W=8, coarse=(2, 32, [1]), fine=(2, 32, [1]), mask_weight=0.5)
    model = MC_Model(sp)
    S.init_cameras_near_gt(model)
    wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0])
    with pytest.raises(McnerfError, match="mask_weight"):
        model((torch.rand(1, 64, 3), torch.tensor([0]), wpts, pts, wpts, pts), 20, "GLOBAL_OPTIM_EPOCH", 0.6)


def test_extension_ops_refuse_host_tensors():
    from mc_nerf_amd import ops
    from mc_nerf_amd._lib import McnerfError
    sig, z, eps = torch.zeros(2, 3, 4), torch.linspace(1, 2, 3), torch.zeros(2, 3)
    with pytest.raises(McnerfError, match=r"mcnerf_ext_front_weight: sig_rgb .*no CPU fallback"):
        ops.front_weight(sig, z, None, eps)
    with pytest.raises(McnerfError, match=r"mcnerf_ext_composite_bwd_front: sig_rgb .*no CPU fallback"):
        ops.composite_bwd_front(sig, z, None, eps, torch.zeros(2, 3), torch.zeros(2))
    with pytest.raises(McnerfError, match=r"mcnerf_ext_gather_alpha: images .*no CPU fallback"):
        ops.gather_alpha(torch.zeros(1, 4, 4, dtype=torch.uint8), [0], [0, 2], torch.zeros(2, dtype=torch.int64))
    with pytest.raises(McnerfError, match=r"mcnerf_ext_mask_loss: fg_c .*no CPU fallback"):
        ops.mask_loss(torch.zeros(2), None, torch.zeros(2), 1.0)
    with pytest.raises(McnerfError, match=r"seg_cam .*host array"):
        from mc_nerf_amd import _ext
        _ext.call("mcnerf_ext_gather_alpha", None, 1, 4, 4, torch.zeros(1, dtype=torch.int32), None, 1, None, 0, None, 0)


def test_entry_points_refuse_before_any_device_work():
    """Raw addresses that are never dereferenced: every refusal below is decided on the host (this machine has no GPU)."""
    from mc_nerf_amd import _ext
    from mc_nerf_amd._lib import McnerfError
    P = 4096                                # a non-null "pointer"
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    # N = 0 / n = 0: no-ops, null pointers allowed
    _ext.call("mcnerf_ext_front_weight", None, None, 0, None, None, 0, 8, None, 0)
    _ext.call("mcnerf_ext_composite_bwd_front", None, None, 0, None, None, None, None, 0, 8, 1, None, None, 0)
    _ext.call("mcnerf_ext_gather_alpha", None, 1, 16, 4, i32(0), i32(0, 0), 1, None, 0, None, 0)
    _ext.call("mcnerf_ext_mask_loss", None, None, None, 0, 1.0, None, None, None, 0)
    bad = [
        ("mcnerf_ext_front_weight", (None, P, 0, None, P, 2, 8, P, 0)),                           # null sig_rgb
        ("mcnerf_ext_front_weight", (P, P, 0, None, P, 2, 0, P, 0)),                              # S = 0
        ("mcnerf_ext_front_weight", (P, P, 3, None, P, 2, 8, P, 0)),                              # z_stride neither 0 nor S
        ("mcnerf_ext_front_weight", (P, P, 0, None, P, -1, 8, P, 0)),                             # N < 0
        ("mcnerf_ext_front_weight", (P, P, 0, None, P, 1 << 21, 1 << 10, P, 0)),                  # N S >= 2^31
        ("mcnerf_ext_composite_bwd_front", (P, P, 0, None, P, P, None, 2, 2049, 1, P, None, 0)),  # S over the LDS bound
        ("mcnerf_ext_composite_bwd_front", (P, P, 0, None, P, None, P, 2, 8, 1, P, None, 0)),     # null d_rgb
        ("mcnerf_ext_composite_bwd_front", (P, P, 0, None, P, P, P, 2, 8, 1, None, None, 0)),     # null output
        ("mcnerf_ext_gather_alpha", (P, 2, 16, 4, i32(0, 2), i32(0, 1, 2), 2, P, 2, P, 0)),       # camera outside [0, C)
        ("mcnerf_ext_gather_alpha", (P, 2, 16, 4, i32(0, 1), i32(0, 2, 1), 2, P, 1, P, 0)),       # not monotone
        ("mcnerf_ext_gather_alpha", (P, 2, 16, 4, i32(0, 1), i32(1, 1, 2), 2, P, 2, P, 0)),       # does not start at 0
        ("mcnerf_ext_gather_alpha", (P, 2, 16, 4, i32(0, 1), i32(0, 1, 3), 2, P, 2, P, 0)),       # does not end at n
        ("mcnerf_ext_gather_alpha", (P, 2, 16, 4, i32(0), i32(0, 2), 0, P, 2, P, 0)),             # K = 0
        ("mcnerf_ext_gather_alpha", (P, 2, 16, 4, i32(*[0] * 65), i32(*range(66)), 65, P, 65, P, 0)),   # K over the bound
        ("mcnerf_ext_gather_alpha", (P, 2, 16, 5, i32(0), i32(0, 2), 1, P, 2, P, 0)),             # channels
        ("mcnerf_ext_gather_alpha", (None, 2, 16, 4, i32(0), i32(0, 2), 1, P, 2, P, 0)),          # null images
        ("mcnerf_ext_mask_loss", (P, None, P, 2, -1.0, P, P, None, 0)),                           # negative weight
        ("mcnerf_ext_mask_loss", (P, None, P, 2, float("nan"), P, P, None, 0)),
        ("mcnerf_ext_mask_loss", (P, P, P, 2, 1.0, P, P, None, 0)),                               # fg_f without d_fg_f
        ("mcnerf_ext_mask_loss", (P, None, None, 2, 1.0, P, P, None, 0)),                         # null alpha
        ("mcnerf_ext_mask_loss", (P, None, P, -1, 1.0, P, P, None, 0)),
    ]
    for name, args in bad:
        with pytest.raises(McnerfError, match=name + r" failed \(-1\): " + name + ": invalid argument"):
            _ext.call(name, *args)


# ------------------------------------------------------------------------------------------------------------------ header / library
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(mcnerf_[a-z_0-9]+)\s*\(", text))


def test_the_extension_header_parses():
    from ctypes import c_float, c_int, c_void_p
    from mc_nerf_amd import _ext, _lib
    assert sorted(_ext.SIGNATURES) == sorted(_declared("mcnerf_ext.h")) and len(_ext.SIGNATURES) == 6
    assert all(n.startswith("mcnerf_ext_") for n in _ext.SIGNATURES) and all(k.startswith("MCNERF_EXT_") for k in _ext.DEFINES)
    assert _ext.ABI_VERSION == 1 and _ext.DEFINES["MCNERF_EXT_MASK_LOSS_OUT"] == 132 and _ext.DEFINES["MCNERF_EXT_BWD_MAX_SAMPLES"] == 2048
    assert not set(_ext.SIGNATURES) & set(_lib.SIGNATURES)
    at = {p[0]: (p[2], p[3]) for p in _ext.PARAMS["mcnerf_ext_gather_alpha"][1]}
    assert at["seg_cam"] == (c_void_p, _lib.HOST) and at["seg_start"] == (c_void_p, _lib.HOST)
    assert at["images"] == (c_void_p, torch.uint8) and at["pix"] == (c_void_p, torch.int64) and at["npix"][1] is None
    assert _ext.SIGNATURES["mcnerf_ext_mask_loss"][1][3:5] == [c_int, c_float]
    assert _ext.McnerfError is _lib.McnerfError and _ext.call is not _lib.call


@pytest.fixture(scope="module")
def built():
    from mc_nerf_amd import build
    if not os.path.isfile(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    core = build.build(verbose=False)
    return core, build.EXT_OUT


def test_one_build_call_makes_both_libraries(built):
    from mc_nerf_amd import _ext, build
    core, ext = built
    assert core == build.OUT and os.path.isfile(core) and os.path.isfile(ext) and os.path.basename(ext) == "libmcnext.so"
    assert not set(build.EXT_SOURCES) & set(build.SOURCES) and "composite.hip" in build.SOURCES
    assert all(os.path.isfile(os.path.join(build.CSRC, s)) for s in build.EXT_SOURCES)
    l = _ext.lib()
    assert l.mcnerf_ext_abi_version() == _ext.ABI_VERSION and l.mcnerf_ext_last_error() is not None


def _exports(lib):
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_each_library_exports_its_own_header_and_nothing_else(built):
    core, ext = built
    ext_syms = {s for s in _exports(ext) if s.startswith("mcnerf_")}
    assert ext_syms == _declared("mcnerf_ext.h")
    core_syms = {s for s in _exports(core) if s.startswith("mcnerf_")}
    assert core_syms == _declared("mcnerf.h") and not [s for s in core_syms if s.startswith("mcnerf_ext_")]


# ------------------------------------------------------------------------------------------------------------------ the references
def test_the_far_plane_sample_takes_the_rest():
    """sum_j w_j is 1 on every ray of the table whose far sample has sigma + eps > -19 (delta = 1e10 makes it opaque), whatever lies in
    front of it -- the planted empty rays have fg = 3e-8 and the same total as the opaque ones: what a mask can supervise is fg."""
    lo, hi = 1.0, 1.0
    for name in R.CASES:
        if R.CASES[name]["N"] > 100:
            continue
        inp = R.make(name)
        z = R.depths(inp["z"], inp["jitter"], inp["sig_rgb"].shape[0]).double()
        delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], dim=-1)
        w = R._weights(delta, inp["sig_rgb"][..., 0].double() + inp["eps"].double())
        # (but where the far sample's sigma + eps is under -19 -- planted rays with a negative draw: softplus * 1e10 is then O(10) or
        #  less and that sample is not opaque; a net reaches such a sigma only by learning it)
        tot = w.sum(1)[(inp["sig_rgb"][:, -1, 0] + inp["eps"][:, -1]) > -19.0]
        if tot.numel():
            lo, hi = min(lo, float(tot.min())), max(hi, float(tot.max()))
        if R.CASES[name]["N"] >= 16 and R.CASES[name]["S"] >= 3:
            fg = w[:, :-1].sum(1)
            assert float(fg[:4].max()) < 1e-6, name                                       # the planted empty rays
            if R.CASES[name]["S"] >= 63 and not R.CASES[name]["rows"]:                    # the planted opaque rays, on the uniform grid
                assert float(fg[4:8].min()) > 0.999, name
    assert 0.99999 < lo and hi < 1.00001, (lo, hi)


@pytest.mark.parametrize("rows", [False, True])
def test_family_b_is_semi_transparent(rows):
    shares = {}
    for shape in M.SHAPES:
        inp = M.variant(shape, "b", rows, True)
        N, S = inp["sig_rgb"].shape[:2]
        if N == 53 and S >= 3:
            shares[shape] = M.semi_transparent_share(M.reference(inp)["fg"])
    print("share of rays with fg in (0.05, 0.95):", {k: round(v, 2) for k, v in shares.items()})
    assert len(shares) == 6 and min(shares.values()) >= M.FRACTION, shares


def test_family_b_keeps_rays_0_to_3_and_family_a_is_the_table():
    a, b, t = M.variant("edge_S65", "a", True, True), M.variant("edge_S65", "b", True, True), R.make("edge_S65_rows")
    for k in ("sig_rgb", "eps", "z", "d_rgb", "jitter"):
        assert torch.equal(a[k], t[k]) and torch.equal(a[k][:4], b[k][:4]), k
    assert not torch.equal(a["sig_rgb"][4:], b["sig_rgb"][4:]) and "\0mask_ref" not in R.CASES
    fa = M.reference(a)["fg"]
    assert float((fa[11:] - 1.0).abs().max()) < 1e-2              # family "a": the drawn rays are all opaque in front of the far plane


@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("shape", ["edge_S3", "edge_S65", "edge_S129", "one_ray"])
def test_fp32_restatement_against_fp64(shape, family):
    """The fp32 restatement (whose error sets the kernels' bar) is itself an fp32-grade statement of the fp64 one, with d_rgb and alone."""
    inp = M.variant(shape, family, True, False)
    for d_rgb in (None, torch.zeros_like(inp["d_rgb"])):
        ref, got = M.reference(inp, d_rgb), M.restated32(inp, d_rgb)
        for k in ("fg", "d_sig_rgb"):
            e, _ = R.worst(got[k], ref[k])
            assert e <= 1e-5 * max(1.0, float(ref[k].abs().max())), (shape, family, k, e)


def test_blob_scene_alpha_is_the_quadrature_weight_sum():
    from mc_nerf_amd import synthetic as S
    g = torch.Generator().manual_seed(3)
    o = torch.nn.functional.normalize(torch.randn(64, 3, generator=g), dim=-1) * 3.0
    d = torch.nn.functional.normalize(-o + 0.6 * torch.randn(64, 3, generator=g), dim=-1)
    rgb, a = S.blob_scene_render(d, o), S.blob_scene_alpha(d, o)
    assert a.shape == (64,) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0 + 1e-6 and float(a.min()) < 0.05 < 0.9 < float(a.max())
    assert float((rgb[a < 1e-3] - 1.0).abs().max()) < 2e-3                # an empty ray is white
    rgba = S.blob_scene_rgba(rgb.unsqueeze(0), a.unsqueeze(0))
    assert rgba.dtype == torch.uint8 and rgba.shape == (1, 64, 4)
    back = rgba[..., :3].float() / 255 * (rgba[..., 3:].float() / 255) + 1 - rgba[..., 3:].float() / 255
    assert float((back[0] - rgb).abs().max()) < 2.5 / 255
