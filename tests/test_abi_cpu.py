"""CPU checks of the C-ABI boundary: the library builds, loads, and exports exactly what
include/mcnerf.h declares (no compute calls - there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "mcnerf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mcnerf_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def built_lib():
    from mc_nerf_amd import build
    return build.build(verbose=False)


def test_header_declares_expected_surface():
    fns = header_functions()
    for must in ["mcnerf_mlp_fwd", "mcnerf_mlp_bwd", "mcnerf_mlp_dw", "mcnerf_composite_fwd", "mcnerf_composite_bwd",
                 "mcnerf_select_fine", "mcnerf_raygen_fwd", "mcnerf_raygen_bwd", "mcnerf_pack_weights"]:
        assert must in fns


def test_library_exports_every_declared_symbol(built_lib):
    l = ctypes.CDLL(built_lib)
    for fn in header_functions():
        assert hasattr(l, fn), f"{fn} declared in include/mcnerf.h but not exported"


def test_ctypes_signatures_cover_header(built_lib):
    from mc_nerf_amd import _lib
    assert sorted(_lib.SIGNATURES) == header_functions()
    l = _lib.lib()
    assert l.mcnerf_abi_version() == _lib.ABI_VERSION


def test_layout_queries_need_no_gpu(built_lib):
    from mc_nerf_amd import ops
    fine, coarse = ops.Net(8, 256, 4), ops.Net(4, 128, 2)
    # reference parameter counts (631 836 / 102 428) plus 16-byte alignment padding
    assert 631836 <= ops.param_count(fine) <= 631836 + 4 * 26
    assert 102428 <= ops.param_count(coarse) <= 102428 + 4 * 18
    offs = ops.param_offsets(fine)
    assert offs[0] == 0 and all(b > a for a, b in zip(offs, offs[1:])) and all(o % 4 == 0 for o in offs)
    assert ops.tile_rows(256) == 64
    assert ops._lib.lib().mcnerf_param_count(3, 100, 1) == -1   # unsupported width


def test_ops_refuse_cpu_tensors(built_lib):
    import torch
    from mc_nerf_amd import ops, _lib
    net = ops.Net(4, 32, 2)
    with pytest.raises(_lib.McnerfError):
        ops.pack_weights(net, torch.zeros(ops.param_count(net)), torch.zeros(ops.packed_count(net)))


def test_general_topology_codes_and_layouts(built_lib):
    """The `skip` argument's mask form (include/mcnerf.h): any `skips` list, SH degree 0 .. 3, 1 .. 10 encoding frequencies.  The flat
    parameter layout of such a net is the reference's state dict (model/net_block.py:51-65) in order, every tensor 16-byte aligned;
    the default topology keeps its legacy codes; the register-chain entry points refuse what they do not take."""
    import numpy as np
    from mc_nerf_amd import ops
    l = ops._lib.lib()
    assert ops.skip_code([4], 8) == 4 and ops.skip_code([], 4) == -1 and ops.skip_code([0, 9], 8) == -1        # (0 and >= depth are not skip layers)
    code = ops.skip_code([2, 4, 6], 8)
    net = ops.Net(8, 64, code)
    assert code >= ops.SKIP_MASK and net.skips == [2, 4, 6] and net.multi_skip and net.deg == 2 and net.n_freqs == 10
    assert [net.in_features(i) for i in range(8)] == [63, 64, 127, 64, 127, 64, 127, 64]
    g = ops.Net(4, 32, ops.skip_code([2], 4, deg=3, n_freqs=6))
    assert (g.skips, g.deg, g.n_sh, g.n_shp, g.n_freqs, g.n_enc) == ([2], 3, 48, 64, 6, 39)
    assert g.fp32_only and net.fp32_only and not ops.Net(8, 256, 4).fp32_only
    for n_ in (net, g, ops.Net(4, 128, ops.skip_code([1, 3], 4, deg=0)), ops.Net(8, 256, 4)):
        offs, shapes = ops.param_offsets(n_), n_.shapes()
        assert len(offs) == len(shapes) == 2 * n_.depth + 8
        end = 0
        for o, shp in zip(offs, shapes):
            assert o % 4 == 0 and end <= o < end + 4          # next 16-byte boundary after the previous tensor
            end = o + int(np.prod(shp))
        assert end <= ops.param_count(n_) < end + 4
        assert ops.packed_count(n_) > 0
    assert ops.param_count(ops.Net(8, 256, ops.skip_code([4], 8))) == ops.param_count(ops.Net(8, 256, 4))
    # refused: degree 4, 11 frequencies, a mask bit at or above the depth; the register-chain sizes of a net they do not take
    assert l.mcnerf_param_count(4, 32, (1 << 8) | 0x80 | (4 << 4)) == -1
    assert l.mcnerf_param_count(4, 32, (1 << 8) | 12) == -1
    assert l.mcnerf_param_count(4, 32, (1 << 8) | (1 << 13)) == -1
    assert l.mcnerf_packed_bytes_16(*net.triple, 2, 0) == -1 and l.mcnerf_packed_bytes_16(*g.triple, 0, 0) == -1
    assert l.mcnerf_packed_bytes_16(8, 256, 4, 2, 0) > 0
    with pytest.raises(ValueError):
        ops.skip_code([2], 4, deg=4)
    with pytest.raises(ValueError):
        ops.skip_code([2], 4, n_freqs=11)


def test_register_chain_dtypes_and_workspace_sizes(built_lib):
    """`dtype` of the `_16` entry points (include/mcnerf.h): 0 = f16, 1 = bf16, 2 = f16x3 (hi + lo planes), 3 = f16x3h (f16x3's chains,
    hi planes only): dtype 3 packs its weights like dtype 2, keeps dtype 2's fp32 sh.2-output tile, and sizes every other workspace
    like dtype 0; anything else is refused."""
    from mc_nerf_amd import ops
    l = ops._lib.lib()
    assert ops.DTYPE16 == {"f16": 0, "bf16": 1, "f16x3": 2, "f16x3h": 3} and set(ops.PRECISIONS) == {"f32", *ops.DTYPE16}
    for depth, width, skip in ((8, 256, 4), (4, 128, 2), (8, 64, 4)):
        for bwd in (0, 1):
            assert l.mcnerf_packed_bytes_16(depth, width, skip, 3, bwd) == l.mcnerf_packed_bytes_16(depth, width, skip, 2, bwd) >= l.mcnerf_packed_bytes_16(depth, width, skip, 0, bwd) > 0      # (slab padding differs between the streams)
        for cap in (1, 4096, 3_200_000):
            for which in (0, 1, 2, 3):
                assert l.mcnerf_ws_bytes_16(depth, width, 3, cap, which) == l.mcnerf_ws_bytes_16(depth, width, 0, cap, which) > 0
                if which != 2:
                    assert l.mcnerf_ws_bytes_16(depth, width, 2, cap, which) == 2 * l.mcnerf_ws_bytes_16(depth, width, 0, cap, which)
            assert l.mcnerf_ws_bytes_16(depth, width, 3, cap, 4) == l.mcnerf_ws_bytes_16(depth, width, 2, cap, 4) == 2 * l.mcnerf_ws_bytes_16(depth, width, 0, cap, 4)
    assert l.mcnerf_packed_bytes_16(8, 256, 4, 4, 0) == -1 and l.mcnerf_ws_bytes_16(8, 256, -1, 4096, 0) == -1 and l.mcnerf_ws_bytes_16(8, 256, 4, 4096, 0) == -1


def test_hi_plane_mode_workspace_layout(built_lib):
    """The layout contract tests/test_mlpx3h_gpu.py compares workspaces under: at capacities around a tile and around a pass, "f16x3h"
    sizes its slots, encoding, ReLU words and dY tile like "f16" (one 16-bit plane: [slot][tile][k-step][2][32][8]), keeps "f16x3"'s
    fp32 sh.2 tile, and "f16x3" holds exactly two such planes per tile -- over the same number of 32-row tiles, whole passes of both
    wave configurations of the chains."""
    from mc_nerf_amd import ops
    for depth, width in ((4, 32), (8, 64), (4, 128), (8, 256), (2, 256)):
        net = ops.Net(depth, width, depth // 2)
        for cap in (1, 31, 32, 33, 257, 4099):
            ws = lambda which, precision: ops.ws_bytes_16(net, cap, which, precision)
            for which in (0, 1, 2, 3):
                assert ws(which, "f16x3h") == ws(which, "f16") > 0
            assert ws(4, "f16x3h") == ws(4, "f16x3") > 0
            for which in (0, 1, 3):
                assert ws(which, "f16x3") == 2 * ws(which, "f16x3h")
            assert ws(2, "f16x3") == ws(2, "f16x3h")
            # the geometry ops.decode_frags_16 / decode_masks_16 / decode_sh_x3 assume: 1 KiB per (tile, k-step) fragment
            tiles, rem = divmod(ws(1, "f16x3h"), 4 * 1024)
            assert rem == 0 and 32 * tiles >= cap and tiles % 8 == 0
            assert ws(0, "f16x3h") == (depth + 2) * tiles * (width // 16) * 1024
            assert ws(2, "f16x3h") == (depth + 2) * tiles * 64 * 4 * max(1, width // 64)
            assert ws(3, "f16x3h") == tiles * 2 * 1024 and ws(4, "f16x3h") == tiles * 4096


# ------------------------------------------------------------------------------------------------------------------ the derived binding
def header_prototypes():
    """{function: number of parameters}, by this file's own regex: the commas between a prototype's parentheses."""
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcnerf.h")).read(), flags=re.S))
    return {name: 0 if args.strip() in ("", "void") else args.count(",") + 1 for name, args in re.findall(r"\b(mcnerf_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", src)}


def header_define(name):
    return int(re.search(rf"^#define {name} (\d+)\b", open(os.path.join(ROOT, "include", "mcnerf.h")).read(), flags=re.M).group(1))


MINI_HEADER = """
/* a comment with a prototype in it: int mcnerf_ghost(float* x, int n); and (parentheses) */
#define MCNERF_ABI_VERSION 7   /* trailing comment (with parentheses) */
#define MCNERF_LIMIT 64
#define MCNERF_MARKER
#define OTHER_THING 3
int mcnerf_abi_version(void);
const char* mcnerf_last_error(void);
long long mcnerf_count(int depth, long long capacity, float thresh);   // int mcnerf_ghost2(int n);
int mcnerf_all(const float* a, float* b, const int32_t* c, int32_t* d, const uint32_t* e, uint32_t* f,
               const int64_t* g, uint64_t* h,
               const uint8_t* i, const void* j, void* stream);
int mcnerf_tables(int n, float* const* params, const float* const* grads, int32_t* const* row_step, const long long* sizes, long long* offsets,
                  MCNERF_HOST const int32_t* seg_cam, MCNERF_HOST const float* host_vals);
"""


def test_parser_covers_every_type_class_on_a_literal_header():
    import torch
    from ctypes import c_char_p, c_float, c_int, c_longlong, c_void_p
    from mc_nerf_amd import _lib
    fns, defines = _lib.parse_header(MINI_HEADER)
    assert defines == {"MCNERF_ABI_VERSION": 7, "MCNERF_LIMIT": 64}
    assert sorted(fns) == ["mcnerf_abi_version", "mcnerf_all", "mcnerf_count", "mcnerf_last_error", "mcnerf_tables"]       # (no ghost)
    assert fns["mcnerf_abi_version"] == (c_int, ()) and fns["mcnerf_last_error"] == (c_char_p, ())
    res, params = fns["mcnerf_count"]
    assert res is c_longlong and [(p[0], p[2], p[3]) for p in params] == [("depth", c_int, None), ("capacity", c_longlong, None), ("thresh", c_float, None)]
    res, params = fns["mcnerf_all"]                                                                   # (a prototype split over three lines)
    assert res is c_int and [p[0] for p in params] == list("abcdefghij") + ["stream"] and all(p[2] is c_void_p for p in params)
    assert [p[3] for p in params] == [torch.float32] * 2 + [torch.int32] * 4 + [torch.int64] * 2 + [torch.uint8] * 3
    assert params[0][1] == "const float*" and params[7][1] == "uint64_t*"
    res, params = fns["mcnerf_tables"]
    assert [p[2] for p in params] == [c_int] + [c_void_p] * 7 and [p[3] for p in params] == [None] + [_lib.HOST] * 7
    assert [p[0] for p in params][-2:] == ["seg_cam", "host_vals"]


@pytest.mark.parametrize("proto, names", [("int mcnerf_bad(const float* x, double y);", ["mcnerf_bad"]),
                                          ("int mcnerf_bad(unsigned n);", ["mcnerf_bad"]),
                                          ("int mcnerf_bad(const char* name);", ["mcnerf_bad"]),
                                          ("int mcnerf_bad(float** table);", ["mcnerf_bad"]),
                                          ("int mcnerf_bad(int);", ["mcnerf_bad"]),
                                          ("double mcnerf_bad(int n);", ["mcnerf_bad"]),
                                          ("int mcnerf_ok(int n);\nint mcnerf_bad(int (*callback)(int), int n);", ["mcnerf_bad"])])
def test_parser_refuses_a_type_it_does_not_know_and_names_the_function(proto, names):
    from mc_nerf_amd import _lib
    with pytest.raises(_lib.McnerfError) as e:
        _lib.parse_header(proto)
    assert all(n in str(e.value) for n in names) and "mcnerf_ok" not in str(e.value)


@pytest.mark.parametrize("name", sorted(header_prototypes()))
def test_every_signature_has_the_headers_argument_count(name):
    from mc_nerf_amd import _lib
    res, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == header_prototypes()[name] == len(_lib.PARAMS[name][1])
    assert res is (ctypes.c_char_p if name == "mcnerf_last_error" else ctypes.c_longlong if name in
                   ("mcnerf_param_count", "mcnerf_packed_count", "mcnerf_packed_bytes_16", "mcnerf_ws_bytes_16", "mcnerf_cap_ws_words") else ctypes.c_int)


def test_the_header_declares_53_entry_points_and_version_7(built_lib):
    from mc_nerf_amd import _lib
    assert len(header_prototypes()) == len(_lib.SIGNATURES) == 53 and sorted(header_prototypes()) == header_functions()
    assert _lib.ABI_VERSION == header_define("MCNERF_ABI_VERSION") == 7 == _lib.lib().mcnerf_abi_version()


def test_float_arguments_by_value_are_c_float():
    from ctypes import c_float
    from mc_nerf_amd import _lib
    at = lambda name: {p[0]: p[2] for p in _lib.PARAMS[name][1]}
    floats = lambda name: [i for i, t in enumerate(_lib.SIGNATURES[name][1]) if t is c_float]
    assert floats("mcnerf_voxel_update") == [3, 4, 5, 6] and [k for k, t in at("mcnerf_voxel_update").items() if t is c_float] == ["bmin", "s", "beta", "one_minus_beta"]
    assert floats("mcnerf_select_fine") == [2, 6] and [k for k, t in at("mcnerf_select_fine").items() if t is c_float] == ["thresh", "sigma_default"]
    assert floats("mcnerf_radam_step") == [6, 7, 8, 9, 10, 11]
    assert [k for k, t in at("mcnerf_radam_step").items() if t is c_float] == ["lr", "beta1", "beta2", "eps", "weight_decay", "step_size"]


def test_ops_constants_are_the_headers_defines():
    from mc_nerf_amd import ops
    for py, c, value in (("SKIP_MASK", "MCNERF_SKIP_MASK", 256), ("MULTICAM_MAXSEG", "MCNERF_MULTICAM_MAXSEG", 64),
                         ("PDF_MAX_SAMPLES", "MCNERF_PDF_MAX_SAMPLES", 1024), ("ERRMAP_MAX_PIXELS", "MCNERF_ERRMAP_MAX_PIXELS", 1 << 26),
                         ("VOXEL_MAX_G", "MCNERF_VOXEL_MAX_G", 1024), ("TRAIN_LOSS_OUT", "MCNERF_TRAIN_LOSS_OUT", 132),
                         ("TRAIN_LOSS_CALIB_OUT", "MCNERF_TRAIN_LOSS_CALIB_OUT", 8), ("TRAIN_LOSS_CALIB_WS", "MCNERF_TRAIN_LOSS_CALIB_WS", 896)):
        assert getattr(ops, py) == header_define(c) == value, py
    api = open(os.path.join(ROOT, "mc_nerf_amd", "csrc", "api.hip")).read()
    for c, internal in (("MCNERF_SKIP_MASK", "MCN_SKIP_MASK"), ("MCNERF_MULTICAM_MAXSEG", "MCN_MULTICAM_MAXSEG"),
                        ("MCNERF_PDF_MAX_SAMPLES", "MCN_PDF_MAX_SAMPLES"), ("MCNERF_TRAIN_LOSS_OUT", "4 + MCN_LOSS_BLOCKS")):
        assert f"static_assert({c} == {internal}," in api
    assert "<= MCNERF_ERRMAP_MAX_PIXELS" in api and "<= MCNERF_VOXEL_MAX_G" in api and "1ll << 26" not in api


def test_call_refuses_host_tensors_by_entry_point_and_parameter(built_lib):
    """A CPU tensor at a float*, an int32_t* and a void* parameter: refused with the names of both before anything reaches C (the
    buffers the calls would have written keep their values; nothing launches, no GPU is needed)."""
    import torch
    from mc_nerf_amd import _lib
    x, w, out = torch.rand(5, 3), torch.ones(4), torch.full((5, 27), -7.0)
    with pytest.raises(_lib.McnerfError, match=r"mcnerf_encode: x .*no CPU fallback"):
        _lib.call("mcnerf_encode", x, w, 5, 4, out, 0)
    with pytest.raises(_lib.McnerfError, match=r"mcnerf_encode: out .*no CPU fallback"):                 # (an address is not checked: x passes)
        _lib.call("mcnerf_encode", 4096, None, 5, 4, out, 0)
    idx, perm, idx2, count = torch.zeros(4, 2, dtype=torch.int32), torch.arange(4), torch.full((4, 2), -7, dtype=torch.int32), torch.full((1,), -7, dtype=torch.int32)
    with pytest.raises(_lib.McnerfError, match=r"mcnerf_cap_gather: idx_in .*no CPU fallback"):
        _lib.call("mcnerf_cap_gather", idx, perm, 4, idx2, count, 0)
    params, packed = torch.zeros(64), torch.full((64,), 7, dtype=torch.uint8)
    with pytest.raises(_lib.McnerfError, match=r"mcnerf_pack_weights_16: packed_fwd .*no CPU fallback"):
        _lib.call("mcnerf_pack_weights_16", 4, 32, 2, None, packed, packed, 0, None, 0)
    with pytest.raises(_lib.McnerfError, match=r"mcnerf_pack_weights_16: params .*no CPU fallback"):
        _lib.call("mcnerf_pack_weights_16", 4, 32, 2, params, packed, packed, 0, None, 0)
    with pytest.raises(_lib.McnerfError, match=r"mcnerf_errmap_sample: seg_cam .*host array"):           # a tensor at a host-table position
        _lib.call("mcnerf_errmap_sample", None, 1, 4, 4, 2, torch.zeros(1, dtype=torch.int32), None, 1, 4, 0.5, None, None, None, 0)
    for args in ((None, None, 0, 4, None), (None, None, 0, 4, None, 0, 0)):                             # (one argument short, one too many)
        with pytest.raises(ValueError):
            _lib.call("mcnerf_encode", *args)
    assert bool((out == -7.0).all()) and bool((idx2 == -7).all()) and int(count) == -7 and bool((packed == 7).all())
