"""Skipping the rays that miss the scene box (sys_param key "ray_bounds_miss"): what needs no GPU.

  the keys         "ray_bounds_miss" is "sample" (the default: aabb mode as it was) or "skip"; anything else is a ValueError naming the
                   key; in "global" mode the key is never read;
  the header       include/mcnerf_hit.h parses with the core header's parser, its names disjoint from the five other headers; the five
                   pinned ABIs are what they were; one build() call makes six libraries, the sixth exporting exactly its header;
  first use        with MCNHIT_LIB pointing nowhere, default-key and aabb + "sample" models are constructed without the library being
                   opened, and a direct call raises "not found ... no CPU fallback";
  refusals         a CPU model refuses a "skip" render with McnerfError; the ops refuse host tensors before the library is opened; N = 0
                   calls are no-ops on null pointers; bad sizes, null pointers and bad boxes are refused ahead of any device work;
  the restatement  tests/ray_skip_ref.py marks the hand-made rays as their table says, lists in torch.nonzero order, and its selection
                   is the oracle's filtered by ray; the rays of the GPU tests are no degenerate case.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import ray_bounds_ref as B
import ray_skip_ref as R
from conftest import make_sys_param

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS, LIST, SELECT, VOXEL = "mcnerf_hit_ray_depths", "mcnerf_hit_list_rays", "mcnerf_hit_select_fine", "mcnerf_hit_voxel_select_rows"
HEADERS = ("mcnerf.h", "mcnerf_ext.h", "mcnerf_reg.h", "mcnerf_geo.h", "mcnerf_box.h", "mcnerf_hit.h")


def _cfg():
    from oracle import mcnerf_oracle as O
    return O.RenderCfg(samples=16, scale=2, coarse=O.NetCfg(2, 32, (1,)), fine=O.NetCfg(2, 32, (1,)))


# ------------------------------------------------------------------------------------------------------------------ the keys
def test_the_default_is_sample_and_skip_is_accepted():
    import dataclasses
    from mc_nerf_amd.model import NeRF_Model
    from mc_nerf_amd.model.render import RenderSettings
    off, sample, skip = (NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", **kw)) for kw in ({}, dict(ray_bounds_miss="sample"), dict(ray_bounds_miss="skip")))
    for m in (off, sample):
        assert m.settings.ray_bounds_miss == "sample" and m.settings.aabb and not m.settings.skip_misses and m.last_ray_hit is None
    assert skip.settings.ray_bounds_miss == "skip" and skip.settings.skip_misses and skip.last_ray_hit is None
    assert list(off.state_dict()) == list(skip.state_dict())            # no new parameter, no new buffer
    fields = [f.name for f in dataclasses.fields(RenderSettings)]
    assert "ray_bounds_miss" in fields and fields[-1] == "want_zexp" and RenderSettings(16, 2, 0.1, 0.0, True).ray_bounds_miss == "sample"
    assert not RenderSettings(16, 2, 0.1, 0.0, True, ray_bounds_miss="skip").skip_misses      # "global": the key changes nothing


@pytest.mark.parametrize("bad", [True, None, "Skip", "drop", 1, ["skip"]])
def test_a_bad_value_names_the_key(bad):
    from mc_nerf_amd.model import NeRF_Model
    with pytest.raises(ValueError, match="ray_bounds_miss"):
        NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", ray_bounds_miss=bad))


@pytest.mark.parametrize("value", ["skip", "never read", None, 7])
def test_the_key_is_never_read_in_global_mode(value):
    from mc_nerf_amd.model import NeRF_Model
    for kw in ({}, dict(ray_bounds="global")):
        m = NeRF_Model(make_sys_param(_cfg(), ray_bounds_miss=value, **kw))
        assert m.settings.ray_bounds_miss == "sample" and not m.settings.skip_misses and m.last_ray_hit is None


# ------------------------------------------------------------------------------------------------------------------ header / library
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(mcnerf_[a-z_0-9]+)\s*\(", text))


def test_the_hit_header_parses_and_its_names_are_its_own():
    from ctypes import c_float, c_int, c_void_p
    from mc_nerf_amd import _box, _ext, _geo, _hit, _lib, _reg
    with open(os.path.join(ROOT, "include", "mcnerf_hit.h")) as f:
        params, defines = _lib.parse_header(f.read())
    assert params == _hit.PARAMS and defines == _hit.DEFINES
    assert sorted(_hit.SIGNATURES) == sorted(_declared("mcnerf_hit.h")) and len(_hit.SIGNATURES) == 6
    assert set(_hit.SIGNATURES) == {"mcnerf_hit_abi_version", "mcnerf_hit_last_error", DEPTHS, LIST, SELECT, VOXEL}
    assert all(n.startswith("mcnerf_hit_") for n in _hit.SIGNATURES) and all(k.startswith("MCNERF_HIT_") for k in _hit.DEFINES)
    assert _hit.ABI_VERSION == 1
    for other in (_lib, _ext, _reg, _geo, _box):
        assert not set(_hit.SIGNATURES) & set(other.SIGNATURES) and not set(_hit.DEFINES) & set(other.DEFINES)
    # each entry point is the one it gates, plus `hit`
    names = lambda b, fn: [p[0] for p in b.PARAMS[fn][1]]
    assert names(_hit, DEPTHS) == names(_box, "mcnerf_box_ray_depths")[:-1] + ["hit", "stream"]
    assert names(_hit, SELECT) == names(_lib, "mcnerf_select_fine")[:-1] + ["hit", "stream"]
    assert names(_hit, VOXEL) == names(_box, "mcnerf_box_voxel_select_rows")[:-1] + ["hit", "stream"]
    assert names(_hit, LIST) == ["hit", "N", "S", "sigma_default", "ray_counts", "ray_offsets", "idx", "count", "out", "stream"]
    for fn in (DEPTHS, LIST, SELECT, VOXEL):
        at = {p[0]: (p[2], p[3]) for p in _hit.PARAMS[fn][1]}
        assert at["hit"] == (c_void_p, torch.int32) and at["N"] == (c_int, None), fn
    assert {p[0]: (p[2], p[3]) for p in _hit.PARAMS[LIST][1]}["sigma_default"] == (c_float, None)
    assert _hit.McnerfError is _lib.McnerfError and _hit.call not in (_lib.call, _ext.call, _reg.call, _geo.call, _box.call)
    # the five pinned ABIs are what they were
    assert _lib.ABI_VERSION == 7 and len(_lib.SIGNATURES) == 53 and len(_ext.SIGNATURES) == 6 and len(_reg.SIGNATURES) == 4
    assert len(_geo.SIGNATURES) == 6 and len(_box.SIGNATURES) == 6 and _box.ABI_VERSION == 1


def test_a_missing_library_is_opened_by_skip_mode_alone():
    env = dict(os.environ, MCNHIT_LIB="/nonexistent/libmcnhit.so", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    code = ("import mc_nerf_amd\n"
            "from mc_nerf_amd import _hit, ops, synthetic as S\n"
            "from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss, NeRF_Model\n"
            "assert _hit.LIB_PATH == '/nonexistent/libmcnhit.so' and not _hit.loaded()\n"
            "sp = S.make_sys_param('cpu', samples=8, scale=2, batch=16, H=8, W=8, coarse=(2, 32, [1]), fine=(2, 32, [1]))\n"
            "NeRF_Model(sp); MC_Model(sp); MC_NeRF_Loss(sp)\n"
            "NeRF_Model(dict(sp, ray_bounds='global', ray_bounds_miss='skip')); NeRF_Model(dict(sp, ray_bounds='aabb'))\n"
            "NeRF_Model(dict(sp, ray_bounds='aabb', ray_bounds_miss='sample')); MC_Model(dict(sp, ray_bounds='aabb', ray_bounds_miss='sample'))\n"
            "NeRF_Model(dict(sp, ray_bounds='aabb', ray_bounds_miss='skip'))\n"
            "assert not _hit.loaded()\n"
            "try:\n    _hit.call('mcnerf_hit_list_rays', None, 0, 8, -20.0, None, None, None, None, None, 0)\n"
            "except _hit.McnerfError as e:\n    assert 'not found' in str(e) and 'no CPU fallback' in str(e)\n"
            "else:\n    raise SystemExit('a missing library did not raise')\n")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)


@pytest.fixture(scope="module")
def built():
    from mc_nerf_amd import build
    if not os.path.isfile(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    core = build.build(verbose=False)
    return core, build.EXT_OUT, build.REG_OUT, build.GEO_OUT, build.BOX_OUT, build.HIT_OUT


def test_one_build_call_makes_six_libraries(built):
    from mc_nerf_amd import _hit, build
    assert built[0] == build.OUT and all(os.path.isfile(p) for p in built) and os.path.basename(built[5]) == "libmcnhit.so"
    assert len(build.LIBRARIES) == 6 and list(build.LIBRARIES)[-1] == "" and "HIT_" in build.LIBRARIES
    assert build.HIT_SOURCES == ["hit_api.hip", "ray_skip.hip"]
    others = set(build.SOURCES) | set(build.EXT_SOURCES) | set(build.REG_SOURCES) | set(build.GEO_SOURCES) | set(build.BOX_SOURCES)
    assert not set(build.HIT_SOURCES) & others
    assert all(os.path.isfile(os.path.join(build.CSRC, s)) for s in build.HIT_SOURCES + build.HIT_HEADERS)
    assert not any(s in build.FILE_FLAGS for s in build.HIT_SOURCES) and not any(f.startswith("-D") for f in build.FLAGS)
    # what ray_skip.hip compiles into the library by inclusion is listed with its headers
    text = open(os.path.join(build.CSRC, "ray_skip.hip")).read()
    assert '#include "ray_bounds.hip"' in text
    for h in ("ray_bounds.hip", "select.hip", "voxel.hip", "mcnerf_compact.h", "mcnerf_ray_skip.h"):
        assert h in build.HIT_HEADERS, h
    l = _hit.lib()
    assert l.mcnerf_hit_abi_version() == _hit.ABI_VERSION and l.mcnerf_hit_last_error() is not None


def test_the_sixth_library_exports_its_own_header(built):
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    from mc_nerf_amd import _hit
    sets = []
    for lib in built:
        out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
        sets.append({l.split()[-1] for l in out.splitlines() if l.strip() and l.split()[-1].startswith("mcnerf_")})
    assert sets[5] == _declared("mcnerf_hit.h") == set(_hit.SIGNATURES)
    for i in range(5):
        assert not sets[i] & sets[5], HEADERS[i]
        assert sets[i] == _declared(HEADERS[i]), HEADERS[i]            # ... and the five others export what they did


def test_the_new_sources_restate_no_shared_body_and_have_no_switches():
    """The hit library's own files define none of the bodies it shares (a definition is a line at column 0 that names the function
    before a `(` and is no declaration), hold no preprocessor conditional and no inline assembly."""
    from mc_nerf_amd import build
    shared = ("box_ray_span", "vox_sample_cell", "vox_cell", "vox_axis", "sel_threshold", "mcn_scan_counts", "mcn_launch_select_scan", "ray_depths_kernel")
    for fn in ("ray_skip.hip", "hit_api.hip", "mcnerf_ray_skip.h"):
        text = open(os.path.join(build.CSRC, fn)).read()
        code = re.sub(r"//.*", "", text)
        assert not re.findall(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", text, flags=re.M), fn
        assert "asm" not in code and "atomic" not in code and "__shared__" not in code, fn
        assert "struct VoxelPred" not in code and "struct SelectPred" not in code, fn
        for line in code.split("\n"):
            for name in shared:
                assert not (re.match(rf"[A-Za-z_][^=;]*\b{name}\s*\(", line) and not line.rstrip().endswith(";")), (fn, name)
    src = {f: open(os.path.join(build.CSRC, f)).read() for f in os.listdir(build.CSRC)}
    assert sum("struct SelectPred" in s for s in src.values()) == 1 and "struct SelectPred" in src["select.hip"]


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_a_cpu_model_refuses_skip_mode():
    from mc_nerf_amd._lib import McnerfError
    from mc_nerf_amd.model import NeRF_Model
    m = NeRF_Model(make_sys_param(_cfg(), ray_bounds="aabb", ray_bounds_miss="skip"))
    d = torch.nn.functional.normalize(torch.randn(4, 3), dim=-1)
    with pytest.raises(McnerfError, match="ray_bounds"):
        m.render_rays_train(d, -3.0 * d, 0, 1.0)
    with pytest.raises(McnerfError, match="ray_bounds"):
        m.render_rays_test(d, -3.0 * d, m.nerf_coarse, m.nerf_fine)


def test_hit_ops_refuse_host_tensors_before_the_library_is_opened(monkeypatch):
    from mc_nerf_amd import _hit, ops
    from mc_nerf_amd._lib import McnerfError
    monkeypatch.setattr(_hit, "lib", lambda: pytest.fail("the library was opened"))
    o, d, g = torch.zeros(2, 3), torch.ones(2, 3), torch.linspace(1, 8, 4)
    hit = torch.ones(2, dtype=torch.int32)
    with pytest.raises(McnerfError, match=DEPTHS + r": rays_o .*no CPU fallback"):
        ops.ray_depths(o, d, B.BOX, 1.0, 8.0, None, g, want_hit=True)
    with pytest.raises(McnerfError, match=LIST + r": hit .*no CPU fallback"):
        ops.list_rays(hit, 4, -20.0)
    with pytest.raises(McnerfError, match=r"hit must be \[N = 2\]"):
        ops.list_rays(torch.ones(2, 1, dtype=torch.int32), 4, -20.0)
    with pytest.raises(McnerfError, match="idx must hold"):
        ops.list_rays(hit, 4, -20.0, idx=torch.zeros(7, 2, dtype=torch.int32))
    with pytest.raises(McnerfError, match=SELECT + r": w_sel .*no CPU fallback"):
        ops.select_fine(torch.ones(2, 4), torch.zeros(1, dtype=torch.int32), 0.1, 2, -20.0, hit=hit)
    with pytest.raises(McnerfError, match=r"hit must be \[N = 2\]"):
        ops.select_fine(torch.ones(2, 4), torch.zeros(1, dtype=torch.int32), 0.1, 2, -20.0, hit=torch.ones(3, dtype=torch.int32))
    grid = ops.VoxelGrid(2, -1.0, 1.0, 0.0, "cpu")
    with pytest.raises(McnerfError, match=VOXEL + r": vox .*no CPU fallback"):
        ops.voxel_select(grid, 0.0, o, d, None, None, -20.0, z_rows=torch.ones(2, 4), hit=hit)
    with pytest.raises(McnerfError, match="hit is taken together with z_rows"):
        ops.voxel_select(grid, 0.0, o, d, g, None, -20.0, hit=hit)


def test_entry_points_refuse_before_any_device_work():
    """Raw addresses that are never dereferenced: every refusal below is decided on the host (no GPU is needed)."""
    from mc_nerf_amd import _hit
    from mc_nerf_amd._lib import McnerfError
    P = 4096                                # a non-null "pointer"
    inf, nan = float("inf"), float("nan")
    box = B.BOX
    # N = 0: no-ops, null pointers allowed
    _hit.call(DEPTHS, None, None, 0, *box, 1.0, 8.0, None, None, 4, None, 0, None, None, None, None, 0)
    _hit.call(LIST, None, 0, 4, -20.0, None, None, None, None, None, 0)
    _hit.call(SELECT, None, None, 0.1, 0, 4, 2, -20.0, None, None, None, None, None, None, 0)
    _hit.call(VOXEL, None, 4, -1.0, 0.5, 0.0, None, None, None, 0, 4, -20.0, None, None, None, None, None, None, 0)
    dep = lambda o=P, d=P, N=2, b=box, near=1.0, far=8.0, g=P, Sc=4, gf=P, Sf=8, zc=P, zf=P, hit=P: (o, d, N, *b, near, far, None, g, Sc, gf, Sf, zc, zf, None, hit, 0)
    lst = lambda hit=P, N=2, S=4, rc=P, ro=P, idx=P, cnt=P: (hit, N, S, -20.0, rc, ro, idx, cnt, None, 0)
    sel = lambda w=P, wmax=P, N=2, Sc=4, scale=2, rc=P, idx=P, cnt=P, hit=P: (w, wmax, 0.1, N, Sc, scale, -20.0, rc, P, idx, cnt, None, hit, 0)
    vox = lambda vox=P, G=4, s=0.5, z=P, N=2, Sc=4, rc=P, hit=P: (vox, G, -1.0, s, 0.0, P, P, z, N, Sc, -20.0, rc, P, P, P, None, hit, 0)
    bad = [
        (DEPTHS, dep(o=None)), (DEPTHS, dep(d=None)), (DEPTHS, dep(g=None)), (DEPTHS, dep(zc=None)), (DEPTHS, dep(hit=None)),
        (DEPTHS, dep(N=-1)), (DEPTHS, dep(Sc=0)), (DEPTHS, dep(Sf=-1)), (DEPTHS, dep(gf=None)), (DEPTHS, dep(zf=None)), (DEPTHS, dep(Sf=0)),
        (DEPTHS, dep(N=1 << 21, Sc=1 << 10)), (DEPTHS, dep(N=1 << 21, Sf=1 << 10)),
        (DEPTHS, dep(b=(0, 0, 0, 0, 1, 1))), (DEPTHS, dep(b=(0, 2, 0, 1, 1, 1))), (DEPTHS, dep(b=(0, 0, 0, 1, 1, nan))), (DEPTHS, dep(b=(-inf, 0, 0, 1, 1, 1))),
        (DEPTHS, dep(near=nan)), (DEPTHS, dep(far=inf)), (DEPTHS, dep(near=8.0)), (DEPTHS, dep(N=0, b=(0, 0, 0, 0, 1, 1))),
        (LIST, lst(hit=None)), (LIST, lst(N=-1)), (LIST, lst(S=0)), (LIST, lst(rc=None)), (LIST, lst(ro=None)), (LIST, lst(idx=None)), (LIST, lst(cnt=None)),
        (LIST, lst(N=1 << 21, S=1 << 10)), (LIST, lst(N=0, S=0)),
        (SELECT, sel(w=None)), (SELECT, sel(wmax=None)), (SELECT, sel(N=-1)), (SELECT, sel(Sc=0)), (SELECT, sel(scale=0)), (SELECT, sel(rc=None)),
        (SELECT, sel(idx=None)), (SELECT, sel(cnt=None)), (SELECT, sel(hit=None)), (SELECT, sel(N=1 << 21, Sc=1 << 9)), (SELECT, sel(N=0, scale=0)),
        (VOXEL, vox(vox=None)), (VOXEL, vox(G=1)), (VOXEL, vox(G=1025)), (VOXEL, vox(s=0.0)), (VOXEL, vox(s=nan)), (VOXEL, vox(z=None)),
        (VOXEL, vox(N=-1)), (VOXEL, vox(Sc=0)), (VOXEL, vox(rc=None)), (VOXEL, vox(hit=None)), (VOXEL, vox(N=1 << 21, Sc=1 << 10)), (VOXEL, vox(N=0, G=1)),
    ]
    for name, args in bad:
        with pytest.raises(McnerfError, match=name + r" failed \(-1\): " + name + ": invalid argument"):
            _hit.call(name, *args)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_marks_the_hand_made_rays_as_their_table_says():
    o, d = B.hand_rays(len(B.HAND))
    hit = R.hit_ref(o, d, B.BOX, B.NEAR, B.FAR)
    assert hit.dtype == torch.int32 and hit.tolist() == [int(h[2]) for h in B.HAND]
    lo, hi, _ = B.span_ref(o, d, B.BOX, B.NEAR, B.FAR)
    inside = [i for i in range(len(B.HAND)) if hit[i] and (float(lo[i]), float(hi[i])) == (B.NEAR, B.FAR)]
    assert 9 in inside                                                  # hit with the span (near, far): the span cannot stand in for the flag
    assert int(hit[13]) == 0 and int(hit[2]) == 0 and not bool(hit[17:].any())          # the graze, a miss, every NaN / inf ray


def test_the_rays_of_the_gpu_tests_are_no_degenerate_case():
    count = lambda o, d: int(R.hit_ref(o, d, B.BOX, B.NEAR, B.FAR).sum())
    d, o = B.model_rays(256)
    assert (count(o, d), 256 - count(o, d)) == (165, 91)
    d, o = B.model_rays(64)
    assert (count(o, d), 64 - count(o, d)) == (34, 30)
    assert count(*B.hand_rays(257)) == 116


@pytest.mark.parametrize("S", [3, 64, 65])
def test_the_restated_lists_are_in_nonzero_order(S):
    g = torch.Generator().manual_seed(S)
    N = 37
    hit = (torch.rand(N, generator=g) < 0.6).to(torch.int32)
    idx, out = R.list_rays_ref(hit, S, -20.0)
    assert idx.shape == (S * int(hit.sum()), 2) and bool((hit[idx[:, 0]] != 0).all())
    key = idx[:, 0] * S + idx[:, 1]
    assert bool((key[1:] > key[:-1]).all())
    assert out.shape == (N, S, 4) and bool((out[..., 0] == -20.0).all()) and bool((out[..., 1:] == 1.0).all())
    # the selection: the oracle's own filtered by ray, for both scales; with all ones the oracle's itself
    from oracle import mcnerf_oracle as O
    w = torch.rand(N, S, generator=g) ** 4
    for scale in (1, 2):
        for thresh in (0.05, 2.0):                                      # (2.0: every weight is below it, the maximum decides)
            got, _ = R.select_fine_ref(w, w.max(), thresh, scale, -20.0, hit)
            assert torch.equal(got, R.oracle_select_on_hits(w, thresh, scale, hit)) and (thresh < 1 or got.shape[0] == scale * int(hit[int(w.argmax()) // S]))
            every, _ = R.select_fine_ref(w, w.max(), thresh, scale, -20.0, torch.ones(N, dtype=torch.int32))
            assert torch.equal(every, O.select_fine(w, O.RenderCfg(weight_thresh=thresh, scale=scale)))
    # NaN weights in a masked ray change nothing
    n0 = int((hit == 0).nonzero()[0])
    w_nan = w.clone()
    w_nan[n0] = float("nan")
    a, _ = R.select_fine_ref(w_nan, w.max(), 0.05, 2, -20.0, hit)
    b, _ = R.select_fine_ref(w, w.max(), 0.05, 2, -20.0, hit)
    assert torch.equal(a, b)
