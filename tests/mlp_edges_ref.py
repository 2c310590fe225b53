"""What tests/test_mlp_edges_gpu.py needs besides the kernels: the workspace geometry of the four MLP precision modes it runs ("f32", "f16x3",
"f16", "bf16"), the operands of the weight-gradient kernels decoded to fp64, and the fp64 GEMMs / column sums those kernels must equal.

Workspace geometry.  Every workspace (save.act / enc / sh / mask, dy, dsh) is [slots][units][bytes of a unit]:
  * f32   : a unit is one ROW, `capacity` of them per slot (row-major fp32, include/mcnerf.h);
  * chains: a unit is one 32-row TILE of fragments, mcn16_cap_tiles(capacity) = ceil(capacity / 256) * 8 of them per slot in all three
            register-chain modes (csrc/mcnerf_16.h; the split-f16 sizes of csrc/mcnerf_x3.h are twice the 16-bit ones, same tile count).
tests/test_mlp_grad_range_gpu.py runs the same helpers in the hi-plane mode "f16x3h" as well (`ALL_MODES`: f16x3's geometry, one stored
plane) and adds the restated gradient scale and its recovery from a stored plane (`grad_scale`, `recover_scale`).
The part of this module that needs no device (`grad_scale`, `recover_scale`, `covered_tiles`, `cap_units`, `dw_reference`) is tested by
tests/test_mlp_edges_ref_cpu.py.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

MODES = ("f32", "f16x3", "f16", "bf16")
ALL_MODES = ("f32", "f16x3", "f16x3h", "f16", "bf16")      # + the hi-plane mode (tests/test_mlpx3h_gpu.py): f16x3's chains, one stored plane
FILL = 0xFF                       # every workspace byte before a launch: NaN in fp32, f16 and bf16


def _ops():
    from mc_nerf_amd import ops
    return ops


def pass_rows(mode, width):
    """Rows of one workgroup pass of the forward / backward: FwdSmem<W>::MT (f32), 32 * mcnx3_waves(W) (f16x3), MCN16_ROWS (f16 / bf16)."""
    if mode == "f32":
        return _ops().tile_rows(width)
    if mode in ("f16x3", "f16x3h"):
        return 32 * (4 if width >= 128 else 8)
    return 256


def unit_rows(mode):
    return 1 if mode == "f32" else 32


def cap_units(mode, capacity):
    """Units per slot of a workspace allocated for `capacity` rows."""
    capacity = max(int(capacity), 1)
    return capacity if mode == "f32" else -(-capacity // 256) * 8


def covered_tiles(rows, R):
    """32-row tiles the chains write for a launch over `rows` rows with R rows per pass: every wave of every pass that runs stores its
    tile, whether or not a listed row falls into it."""
    return -(-rows // R) * (R // 32)


def covered_units(mode, rows, R):
    """Units of a workspace a launch over `rows` rows may write: the rows themselves (f32: every store is predicated on its row), the
    tiles of the passes that run (chains)."""
    return rows if mode == "f32" else covered_tiles(rows, R)


SG_LOG2, SG_MAX_LOG2, GMAX_LIMIT = 4, 100, 3e38              # MCN16_SG_LOG2, the clamp of the exponent and the bound of the word (csrc/mcnerf_16.h)


def grad_scale(gmax):
    """mcn16_grad_scale (csrc/mcnerf_16.h), the whole function on the fp32 value of `gmax`: the power of two the chains' backward
    multiplies dY by and their weight-gradient kernels divide by.  `(gmax > 0.f && gmax < 3e38f) ? exp2f(fminf(4 - ceilf(log2f(gmax)),
    100.f)) : 1.f`: 1 for a word that is zero, negative, NaN or at / above 3e38f; the exponent clamped at 100 (a word below 2^-96).
    log2f is an fp32 function, restated as the fp64 log2 rounded to fp32: exact at a power of two, and just ABOVE 2^k it still returns k
    wherever log2(1 + eps) is below half an ulp of k (the fp32 neighbour above 2^k: every |k| >= 2; up to 2^k (1 + 2.7e-6) at |k| >= 64).
    There the scale does not halve yet and gmax * SG exceeds 2^4 by that factor: harmless for the range (the planes have 4096x headroom),
    but it is what both kernels compute, so it is what the planes are decoded with (measured on an MI355X: the device's log2f rounds the
    same way at 2^-96, 2^-95, 2^0, 2^4, 2^100 and both neighbours of each, tests/test_mlp_grad_range_gpu.py)."""
    g = np.float32(gmax)
    if not (g > np.float32(0) and g < np.float32(GMAX_LIMIT)):
        return 1.0
    return 2.0 ** min(SG_LOG2 - math.ceil(float(np.float32(math.log2(float(g))))), SG_MAX_LOG2)


def sigma_column(mode, dsh, rows):
    """Column 27 of the stored dsh workspace (d sigma at the run's scale), rows [0, rows), fp64: row-major in f32, ops.decode_frags_16
    in the chains (hi + lo in f16x3, the one plane otherwise)."""
    if mode == "f32":
        return dsh.view(-1, 32)[:rows, 27].double().cpu()
    return _ops().decode_frags_16(dsh, 1, 32, rows, mode)[0][:, 27].double().cpu()


def recover_scale(mode, dsh, d_out_rows):
    """log2 of the gradient scale a run USED, from what it stored: column 27 of `dsh` holds d_out[row, 0] * SG rounded to the mode's 16
    bits (mlp16_bwd.hip / mlp_x3_bwd.hip `dsg = go[0] * sg`; f32: d_out[row, 0] itself, SG = 1).  `d_out_rows` [rows, 4]: the output
    gradient of the listed rows in list order.  Taken at the row with the largest |d_out[row, 0]|; the ratio must be a power of two to
    2^-7 (bf16 rounds to 2^-9, f16 to 2^-12; a word that overstates the maximum by 2^20 leaves an f16 value 2^-24 / 2^-17 = 2^-7 of
    itself per quantum, half of that after rounding)."""
    g = d_out_rows[:, 0].double().cpu()
    i = int(g.abs().argmax())
    want, got = float(g[i]), float(sigma_column(mode, dsh, g.shape[0])[i])
    assert want != 0 and math.isfinite(want), f"row {i}: d_out[row, 0] = {want} says nothing about the scale"
    ratio = got / want
    assert math.isfinite(ratio) and ratio > 0, f"{mode}: dsh column 27 of row {i} is {got} for d_out {want}"
    e = round(math.log2(ratio))
    assert abs(ratio / 2.0 ** e - 1.0) <= 2.0 ** -7, f"{mode}: dsh / d_out = {ratio!r} at row {i} is no power of two (nearest 2^{e})"
    return e


def workspaces(net, r):
    """(name, tensor, slots) of the six workspaces of a run (`r.save`, `r.dy`, `r.dsh`)."""
    n = net.depth + 2
    return [("act", r.save.act, n), ("enc", r.save.enc, 1), ("sh", r.save.sh, 1), ("mask", r.save.mask, n), ("dy", r.dy, n), ("dsh", r.dsh, 1)]


def unit_bytes(mode, buf, slots, capacity):
    """A workspace as bytes [slots][units][bytes of a unit]."""
    return buf.view(torch.uint8).view(slots, cap_units(mode, capacity), -1)


def fill_ff(bufs):
    for b in bufs:
        b.view(torch.uint8).fill_(FILL)


def tile_planes(mode, buf, slots, width, tile):
    """Tile `tile` of a chain mode's fragment workspace as stored, no plane added to another: [slots, parts, k-steps, 2, 32 rows, 8] fp32
    (parts: hi and lo in f16x3, one otherwise; the layouts of ops.decode_frags_16)."""
    dt = torch.bfloat16 if mode == "bf16" else torch.float16
    parts, ks = (2 if mode == "f16x3" else 1), width // 16
    return buf.view(dt).view(slots, -1, parts, ks, 2, 32, 8)[:, tile].float()


def operands(mode, net, save, dy, dsh, rows, sg):
    """X and dY of every layer as the weight-gradient kernel of `mode` reads them, rows [0, rows), fp64, on the workspaces' device:
    .enc [rows, 63], .dsh [rows, 32] (column 27: d sigma) and, one slot at a time (the workspaces can be GBs), .act(l), .dy(l) [rows, W]
    for slot l of depth + 2 (trunk layers, then the sigma and the sh hidden layer).  f32: the row-major views of
    tests/test_a_ops_gpu.py::test_mlp_dw_at_scale.  Chains: ops.decode_frags_16 with the mode's scales undone -- X / SPLIT_SCALE_X in
    f16x3 (hi + lo) and f16x3h (the hi plane), X as stored in f16 / bf16, dY and dsh / sg in all three (sg = grad_scale(max|d_out|))."""
    D, W = net.depth, net.width
    if mode == "f32":
        cap = save.capacity
        act_v, dy_v = save.act.view(D + 2, cap, W), dy.view(D + 2, cap, W)
        return SimpleNamespace(enc=save.enc.view(cap, 64)[:rows, :63].double(), dsh=dsh.view(cap, 32)[:rows].double(),
                               act=lambda l: act_v[l, :rows].double(), dy=lambda l: dy_v[l, :rows].double())
    ops = _ops()
    sx = ops.SPLIT_SCALE_X if mode in ("f16x3", "f16x3h") else 1.0
    na, ny = save.act.numel() // (D + 2), dy.numel() // (D + 2)
    return SimpleNamespace(enc=ops.decode_frags_16(save.enc, 1, 64, rows, mode)[0][:, :63].double() / sx,
                           dsh=ops.decode_frags_16(dsh, 1, 32, rows, mode)[0].double() / sg,
                           act=lambda l: ops.decode_frags_16(save.act[l * na:(l + 1) * na], 1, W, rows, mode)[0].double() / sx,
                           dy=lambda l: ops.decode_frags_16(dy[l * ny:(l + 1) * ny], 1, W, rows, mode)[0].double() / sg)


def dw_reference(depth, skip, opnd):
    """Every parameter gradient of a net with `depth` trunk layers and the skip layer `skip` as the fp64 GEMM dY^T X / column sum of dY over
    the operands `opnd` (see `operands`), by the reference's parameter names: 2 depth + 8 tensors, on the CPU."""
    D = depth
    ref = {}
    for l in range(D):
        x = opnd.enc if l == 0 else (torch.cat([opnd.enc, opnd.act(l - 1)], 1) if l == skip else opnd.act(l - 1))
        g = opnd.dy(l)
        ref[f"xyz_encoding_{l + 1}.0.weight"], ref[f"xyz_encoding_{l + 1}.0.bias"] = g.t() @ x, g.sum(0)
    trunk = opnd.act(D - 1)
    g = opnd.dy(D)
    ref["sigma.0.weight"], ref["sigma.0.bias"] = g.t() @ trunk, g.sum(0)
    g = opnd.dy(D + 1)
    ref["sh.0.weight"], ref["sh.0.bias"] = g.t() @ trunk, g.sum(0)
    ref["sh.2.weight"], ref["sh.2.bias"] = opnd.dsh[:, :27].t() @ opnd.act(D + 1), opnd.dsh[:, :27].sum(0)
    ref["sigma.2.weight"], ref["sigma.2.bias"] = opnd.dsh[:, 27:28].t() @ opnd.act(D), opnd.dsh[:, 27:28].sum(0)
    return {k: v.cpu() for k, v in ref.items()}
