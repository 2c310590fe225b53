#!/usr/bin/env python3
"""Records tests/golden/ray_preamble_lens.npz: what the two lens ray-batch kernels (lens_ray_batch_fwd, lens_ray_batch_bwd) give for
the ray batch of make_ray_preamble.py (its `inputs()`, SEG_START, SEG_CAMS, BATCH_SEED) and a fixed non-zero lens [7,2], on an MI355X.

    MCNERF_LIB=<libmcnerf.so of the commit to record from> python tests/golden/make_ray_preamble_lens.py [out.npz]

The committed file was recorded from the library of the commit BEFORE the pinhole and the lens kernels became one body with a lens
option, so tests/test_ray_preamble_gpu.py holds the merged body to the bits of the lens copy it replaced, at k != 0.  The file holds
the lens and the outputs only: the batch is the "in.b_*" entries of ray_preamble.npz (checked equal to `inputs()` before recording).
`run` is also what the test calls: the cases exist once.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_ray_preamble as base  # noqa: E402

LENS_SEED = 11
K1_MAX, K2_MAX = 0.08, 0.01         # the bounds of tests/lens_ref.py


def lens():
    """lens [7,2] (k1, k2), uniform in [-K1_MAX, K1_MAX] x [-K2_MAX, K2_MAX]."""
    g = torch.Generator().manual_seed(LENS_SEED)
    u = torch.rand(base.C, 2, generator=g) * 2.0 - 1.0
    return np.ascontiguousarray((u * torch.tensor([K1_MAX, K2_MAX])).float().numpy())


def run(z, dev):
    """{case name: host numpy array} of every lens kernel output; `z` holds the "in.b_*" entries of ray_preamble.npz and "in.lens"."""
    from mc_nerf_amd import ops
    t = {k[3:]: torch.from_numpy(v.astype(np.int64) if v.dtype == np.int32 else v).to(dev) for k, v in z.items()
         if k.startswith("in.b_") or k == "in.lens"}
    word = lambda s: torch.tensor([s], dtype=torch.int32, device=dev)
    out = {}
    for draw in ("injected", "drawn"):
        for images in (None, t["b_images"]):
            kw = dict(pix=t["b_pix"]) if draw == "injected" else dict(seed=word(base.BATCH_SEED))
            res = ops.lens_ray_batch_fwd(t["b_pose"], t["b_kinv"], t["lens"], base.SEG_CAMS["distinct"], base.SEG_START, base.BH, base.BW,
                                         images=images, **kw)
            for key, v in zip(("pix", "d", "o", "gt"), res):
                if v is not None:
                    out[f"lens_ray_batch_fwd.{draw}.{'images' if images is not None else 'no_images'}.{key}"] = v
    for table, cams in base.SEG_CAMS.items():
        res = ops.lens_ray_batch_bwd(t["b_pose"], t["b_kinv"], t["lens"], cams, base.SEG_START, base.BW, t["b_pix"], t["b_g_d"], t["b_g_o"])
        for key, v in zip(("d_pose", "d_kinv", "d_lens"), res):
            out[f"lens_ray_batch_bwd.{table}.{key}"] = v
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_not_inert(z, out, dev):
    """The fixture cannot pass on a lens that does nothing: every non-empty segment's directions differ from the pinhole kernel's,
    every camera that owns rays has a non-zero d_lens row, and everything is finite."""
    from mc_nerf_amd import ops
    t = lambda k: torch.from_numpy(z["in." + k].astype(np.int64) if z["in." + k].dtype == np.int32 else z["in." + k]).to(dev)
    assert np.abs(z["in.lens"][:, 0]).max() <= K1_MAX and np.abs(z["in.lens"][:, 1]).max() <= K2_MAX
    for draw in ("injected", "drawn"):
        kw = dict(pix=t("b_pix")) if draw == "injected" else dict(seed=torch.tensor([base.BATCH_SEED], dtype=torch.int32, device=dev))
        pix, d, o, _ = ops.ray_batch_fwd(t("b_pose"), t("b_kinv"), base.SEG_CAMS["distinct"], base.SEG_START, base.BH, base.BW, **kw)
        d = d.cpu().numpy()
        assert np.array_equal(pix.cpu().numpy(), out[f"lens_ray_batch_fwd.{draw}.no_images.pix"])
        assert np.array_equal(o.cpu().numpy(), out[f"lens_ray_batch_fwd.{draw}.no_images.o"])
        for lo, hi in zip(base.SEG_START, base.SEG_START[1:]):
            assert hi == lo or not np.array_equal(d[lo:hi], out[f"lens_ray_batch_fwd.{draw}.no_images.d"][lo:hi]), (draw, lo, hi)
    for table, cams in base.SEG_CAMS.items():
        owners = {c for c, lo, hi in zip(cams, base.SEG_START, base.SEG_START[1:]) if hi > lo}
        d_lens = out[f"lens_ray_batch_bwd.{table}.d_lens"]
        for c in range(base.C):
            assert bool(np.all(d_lens[c] != 0)) == (c in owners), (table, c, d_lens[c])
    for k, v in out.items():
        assert v.dtype.kind != "f" or np.isfinite(v).all(), k


if __name__ == "__main__":
    from mc_nerf_amd import _lib
    dev = torch.device("cuda:0")
    committed = np.load(os.path.join(HERE, "ray_preamble.npz"))
    z = {k: v for k, v in base.inputs().items() if k.startswith("in.b_")}
    for k, v in z.items():
        assert np.array_equal(v, committed[k]), f"{k} of inputs() is not what ray_preamble.npz holds"
    z["in.lens"] = lens()
    out = run(z, dev)
    check_not_inert(z, out, dev)
    out["in.lens"] = z["in.lens"]
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ray_preamble_lens.npz")
    out = {k: v.astype(np.int32) if v.dtype == np.int64 else v for k, v in out.items()}          # (every id is < 2^31: half the bytes)
    np.savez_compressed(path, **out)
    print(f"recorded {len(out)} arrays from {_lib.LIB_PATH} -> {path} ({os.path.getsize(path)} bytes)")
