#!/usr/bin/env python3
"""Records tests/golden/ray_preamble.npz: the inputs of tests/test_ray_preamble_gpu.py and what the six kernels of the ray preamble
(sample_perm, raygen_fwd, raygen_bwd, gather_gt, ray_batch_fwd, ray_batch_bwd) give for them, on an MI355X.

    MCNERF_LIB=<libmcnerf.so of the commit to record from> python tests/golden/make_ray_preamble.py [out.npz]

MCNERF_LIB selects the library (mc_nerf_amd/_lib.py), one process per library.  The committed file was recorded from the library of
the commit BEFORE the per-ray arithmetic moved into csrc/mcnerf_rays.h, so the test holds the shared functions to the bits of the
two hand-kept copies they replaced.  `run` is also what the test calls: the cases exist once.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PERM_CASES = [(1, 1), (2, 2), (35, 35), (1000, 257), (640000, 1024)]
PERM_SEEDS = [42, 0x7FFFFFF0]
FWD_COUNTS = [1, 63, 64, 65, 256, 257]          # of the W = 40, H = 30 camera; around the wave and the 256-thread block
BWD_COUNTS = [1, 63, 64, 65, 256]               # one workgroup: one fixed order of the atomics
C, BH, BW = 7, 12, 20                           # the ray batch: 7 cameras, 12 x 20 images
SEG_START = [0, 86, 172, 172, 257]              # 86 / 86 / (empty) / 85 rays
SEG_CAMS = {"distinct": [5, 0, 3, 2], "shared": [5, 0, 3, 5]}       # "shared": camera 5 owns two segments
BATCH_SEED = 0x7FFFFFF0                         # (the segment keys wrap past 2^32 from segment 1 on)


def inputs():
    """The fixed inputs (host numpy arrays): the pose / kinv of tests/test_a_ops_gpu.py::test_raygen, the 20 x 30 images of its
    gather_gt test, and 7 cameras of a ball for the ray batch."""
    from mc_nerf_amd import synthetic as S
    from oracle import mcnerf_oracle as O
    g = torch.Generator().manual_seed(5)
    z = {"pose": O.se3_to_SE3(torch.randn(1, 6, generator=g) * 0.6)[0],
         "kinv": torch.tensor([[55.0, 0, 20.3], [0, 52.0, 14.1], [0, 0, 1]]).inverse(),
         "pix": torch.randperm(30 * 40, generator=g)[:257],
         "g_d": torch.randn(257, 3, generator=g), "g_o": torch.randn(257, 3, generator=g)}
    g = torch.Generator().manual_seed(0)
    z["img4"] = torch.randint(0, 256, (20 * 30, 4), dtype=torch.uint8, generator=g)
    z["img3"] = torch.randint(0, 256, (20 * 30, 3), dtype=torch.uint8, generator=g)
    z["img_pix"] = torch.randperm(20 * 30, generator=g)[:257]
    g = torch.Generator().manual_seed(1)
    pose, K, _ = S.ball_cameras(0, H=BH, W=BW)
    sel = torch.randperm(pose.shape[0], generator=g)[:C]
    z["b_pose"] = pose[sel].float()
    z["b_kinv"] = torch.linalg.inv(K[sel].double()).float() * (1.0 + 0.05 * torch.randn(C, 3, 3, generator=g))
    z["b_images"] = torch.randint(0, 256, (C, BH * BW, 4), dtype=torch.uint8, generator=g)
    z["b_pix"] = torch.randint(0, BH * BW, (257,), generator=g)
    z["b_g_d"], z["b_g_o"] = torch.randn(257, 3, generator=g), torch.randn(257, 3, generator=g)
    return {"in." + k: np.ascontiguousarray(v.numpy()) for k, v in z.items()}


def run(z, dev):
    """{case name: host numpy array} of every kernel output for the inputs `z` (the "in." entries of the fixture)."""
    from mc_nerf_amd import ops
    t = {k[3:]: torch.from_numpy(v.astype(np.int64) if v.dtype == np.int32 else v).to(dev) for k, v in z.items() if k.startswith("in.")}
    word = lambda s: torch.tensor([s], dtype=torch.int32, device=dev)
    out = {}
    for n, batch in PERM_CASES:
        for seed in PERM_SEEDS:
            out[f"sample_perm.{n}.{batch}.{seed}"] = ops.sample_perm(n, batch, dev, word(seed))
    full = torch.arange(35, device=dev)
    for name, pix, W in [("7x5", full, 7)] + [(f"40x30.{n}", t["pix"][:n].contiguous(), 40) for n in FWD_COUNTS]:
        out[f"raygen_fwd.{name}.d"], out[f"raygen_fwd.{name}.o"] = ops.raygen_fwd(t["pose"], t["kinv"], pix, W)
    for n in BWD_COUNTS:
        out[f"raygen_bwd.{n}.d_pose"], out[f"raygen_bwd.{n}.d_kinv"] = ops.raygen_bwd(
            t["pose"], t["kinv"], t["pix"][:n].contiguous(), 40, t["g_d"][:n].contiguous(), t["g_o"][:n].contiguous())
    for ch in (3, 4):
        out[f"gather_gt.{ch}"] = ops.gather_gt(t[f"img{ch}"], t["img_pix"])
    cams = SEG_CAMS["distinct"]
    for draw in ("injected", "drawn"):
        for images in (None, t["b_images"]):
            kw = dict(pix=t["b_pix"]) if draw == "injected" else dict(seed=word(BATCH_SEED))
            res = ops.ray_batch_fwd(t["b_pose"], t["b_kinv"], cams, SEG_START, BH, BW, images=images, **kw)
            for key, v in zip(("pix", "d", "o", "gt"), res):
                if v is not None:
                    out[f"ray_batch_fwd.{draw}.{'images' if images is not None else 'no_images'}.{key}"] = v
    for table, cams in SEG_CAMS.items():
        out[f"ray_batch_bwd.{table}.d_pose"], out[f"ray_batch_bwd.{table}.d_kinv"] = ops.ray_batch_bwd(
            t["b_pose"], t["b_kinv"], cams, SEG_START, BW, t["b_pix"], t["b_g_d"], t["b_g_o"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


if __name__ == "__main__":
    from mc_nerf_amd import _lib
    z = inputs()
    z.update(run(z, torch.device("cuda:0")))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ray_preamble.npz")
    z = {k: v.astype(np.int32) if v.dtype == np.int64 else v for k, v in z.items()}          # (every id is < 2^31: half the bytes)
    np.savez_compressed(path, **z)
    print(f"recorded {len(z)} arrays from {_lib.LIB_PATH} -> {path} ({os.path.getsize(path)} bytes)")
