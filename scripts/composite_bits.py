"""Records the BITS of the one-wave-per-ray weight kernels of the three libraries, for a change that must leave them alone (the
composite backward and the fp64 weight sweep are defined once, csrc/mcnerf_composite.h, and compiled into each library).

    python scripts/composite_bits.py [out.txt]        (needs the GPU)

A fresh process per library set: MCNERF_LIB, MCNEXT_LIB and MCNREG_LIB select the builds (mc_nerf_amd/_lib.py, _ext.py, _reg.py), e.g.
the parent commit's; run once per set and compare the two files line for line.  The kernels use no atomics besides the max word,
so two builds of the same arithmetic give the same text.

One line per input, the first 16 hex digits of the sha1 of each output's bytes:
  * every variant of tests/mask_ref.SHAPES x family x depth form x white_back (tests/distortion_ref.variant: 80 variants) and every
    case of tests/composite_ref.CASES (d_fg, d_dist drawn as the tests draw them);
  * fw = front_weight; dist, mom = distortion_fwd; the backward d_sig_rgb and its gmax word (`/`) in the four modes of
    composite_bwd_w: none, fg, dist, both; core = composite_bwd; ext_none, ext_fg = composite_bwd_front without and with d_fg.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import composite_ref as R  # noqa: E402
import distortion_ref as D  # noqa: E402
import mask_ref as M  # noqa: E402
from mc_nerf_amd import ops  # noqa: E402


def sha(t):
    return hashlib.sha1(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def line(key, inp, dev):
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    grid, zr = (None, d["z"]) if d["z"].dim() == 2 else (d["z"], None)
    args, wb = (d["sig_rgb"], grid, d["jitter"], d["eps"]), d["white_back"]
    dist, mom = ops.distortion_fwd(*args, D.NEAR, D.FAR, z_rows=zr)
    out = [("fw", sha(ops.front_weight(*args, z_rows=zr))), ("dist", sha(dist)), ("mom", sha(mom))]
    pair = lambda r: sha(r[0]) + "/" + sha(r[1])
    for mode, d_fg, d_dist in (("none", None, None), ("fg", d["d_fg"], None), ("dist", None, d["d_dist"]), ("both", d["d_fg"], d["d_dist"])):
        out.append((mode, pair(ops.composite_bwd_w(*args, d["d_rgb"], d_fg, d_dist, mom, D.NEAR, D.FAR, wb, True, z_rows=zr))))
    out.append(("core", pair(ops.composite_bwd(*args, d["d_rgb"], wb, True, z_rows=zr))))
    out.append(("ext_none", pair(ops.composite_bwd_front(*args, d["d_rgb"], None, wb, True, z_rows=zr))))
    out.append(("ext_fg", pair(ops.composite_bwd_front(*args, d["d_rgb"], d["d_fg"], wb, True, z_rows=zr))))
    torch.cuda.synchronize()
    return f"{key}: " + " ".join(f"{k} {v}" for k, v in out)


def main():
    if not torch.cuda.is_available():
        sys.exit("composite_bits.py runs the kernels on the GPU; there is none here")
    dev = torch.device("cuda:0")
    lines = []
    for shape in M.SHAPES:
        for family in ("a", "b"):
            for rows in (False, True):
                for wb in (True, False):
                    lines.append(line(f"{shape} {family} {'rows' if rows else 'grid'} wb{int(wb)}", D.variant(shape, family, rows, wb), dev))
    for name, c in R.CASES.items():
        inp = R.make(name)
        N = inp["d_rgb"].shape[0]
        inp["d_fg"] = torch.randn(N, generator=torch.Generator().manual_seed(c["seed"] + 77))
        inp["d_dist"] = torch.randn(N, generator=torch.Generator().manual_seed(c["seed"] + 177))
        lines.append(line(f"case {name}", inp, dev))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
