"""Builds mc_nerf_amd/libmcnerf.so and, beside it, the extension library mc_nerf_amd/libmcnext.so, the regulariser library
mc_nerf_amd/libmcnreg.so, the geometry library mc_nerf_amd/libmcngeo.so and the bounds library mc_nerf_amd/libmcnbox.so (hipcc,
gfx950 only) in-tree.

    python -m mc_nerf_amd.build [--force]

hipcc cross-compiles without a GPU; the .so travels to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libmcnerf.so")
SOURCES = ["api.hip", "pack.hip", "mlp_fwd.hip", "mlp_bwd.hip", "mlp_dw.hip", "pack16.hip", "mlp16_fwd.hip", "mlp16_bwd.hip", "mlp16_dw.hip", "mlp_x3_fwd.hip", "mlp_x3_bwd.hip", "mlp_x3_dw.hip", "composite.hip", "sample_pdf.hip", "select.hip", "rays.hip", "voxel.hip", "optim.hip", "optim_rows.hip", "camera.hip", "color_calib.hip", "errmap.hip", "lens.hip"]
HEADERS = ["mcnerf_common.h", "mcnerf_kernels.h", "mcnerf_wave.h", "mcnerf_composite.h", "mcnerf_16.h", "mcnerf_x3.h", "mcnerf_launch.h", "mcnerf_voxel.h",
           "mcnerf_sample_pdf.h", "mcnerf_multicam.h", "mcnerf_colorcal.h", "mcnerf_errmap.h", "mcnerf_maxkey.h", "mcnerf_compact.h", "mcnerf_hash.h", "mcnerf_rays.h", "mcnerf_lens.h", "mcnerf_optim_rows.h", os.path.join("..", "..", "include", "mcnerf.h")]
# The extension library (include/mcnerf_ext.h): opt-in features whose entry points are not part of the core ABI.  Its
# objects share the object directory; nothing of it is linked into libmcnerf.so and it links none of the core's objects.
EXT_OUT = os.path.join(HERE, "libmcnext.so")
EXT_SOURCES = ["ext_api.hip", "mask.hip"]
EXT_HEADERS = ["mcnerf_common.h", "mcnerf_wave.h", "mcnerf_composite.h", "mcnerf_multicam.h", "mcnerf_mask.h", os.path.join("..", "..", "include", "mcnerf.h"),
               os.path.join("..", "..", "include", "mcnerf_ext.h")]
# The regulariser library (include/mcnerf_reg.h): the extension library's ABI is pinned too, so the distortion loss has
# a third library, built the same way.  None of its objects is linked into the other two and it links none of theirs.
REG_OUT = os.path.join(HERE, "libmcnreg.so")
REG_SOURCES = ["reg_api.hip", "distortion.hip"]
REG_HEADERS = ["mcnerf_common.h", "mcnerf_wave.h", "mcnerf_composite.h", "mcnerf_distortion.h", os.path.join("..", "..", "include", "mcnerf_reg.h")]
# The geometry library (include/mcnerf_geo.h): the regulariser library's ABI is pinned as well, so depth supervision has
# a fourth library, built the same way.  None of its objects is linked into the other three and it links none of theirs.
GEO_OUT = os.path.join(HERE, "libmcngeo.so")
GEO_SOURCES = ["geo_api.hip", "depth.hip"]
GEO_HEADERS = ["mcnerf_common.h", "mcnerf_wave.h", "mcnerf_composite.h", "mcnerf_multicam.h", "mcnerf_depth.h", os.path.join("..", "..", "include", "mcnerf.h"),
               os.path.join("..", "..", "include", "mcnerf_geo.h")]
# The bounds library (include/mcnerf_box.h): the geometry library's ABI is pinned too, so per-ray sample bounds have a
# fifth library, built the same way.  The sampler's device code reaches it through mcnerf_sample_pdf.h and the voxel kernels by
# ray_bounds.hip including voxel.hip (listed with the headers: a change of it recompiles ray_bounds.hip); none of its objects is
# linked into the other four and it links none of theirs.
BOX_OUT = os.path.join(HERE, "libmcnbox.so")
BOX_SOURCES = ["box_api.hip", "ray_bounds.hip"]
BOX_HEADERS = ["mcnerf_common.h", "mcnerf_kernels.h", "mcnerf_wave.h", "mcnerf_voxel.h", "voxel.hip", "mcnerf_compact.h", "mcnerf_maxkey.h",
               "mcnerf_sample_pdf.h", "mcnerf_ray_bounds.h", os.path.join("..", "..", "include", "mcnerf.h"),
               os.path.join("..", "..", "include", "mcnerf_box.h")]
# the f16x3 chains: a layer body is ~400 MFMAs with its epilogue slices, fully unrolled (beyond hipcc's default pragma-unroll budget);
# their 256-wide instantiations run one wave per SIMD with 512 registers, where hipcc would otherwise put the MFMA
# accumulators in AGPRs (every epilogue read then costs a v_accvgpr_read behind a full MFMA drain)
FILE_FLAGS = {s: ["-mllvm", "-pragma-unroll-threshold=200000", "-mllvm", "-amdgpu-mfma-vgpr-form"] for s in ("mlp_x3_fwd.hip", "mlp_x3_bwd.hip")}
# -fno-slp-vectorize: hipcc's SLP vectoriser packs adjacent scalar fp32 multiplies / adds of the layer epilogues into v_pk_mul_f32 /
# v_pk_add_f32, which cost more beside MFMAs than the scalar pairs they replace (MI355X_MICROARCH.md, issue-cost table); same-box A/B:
# f16x3 saving forward 12.03 -> 11.60 ms (256-wide), 3.17 -> 3.08 (128-wide), 128-wide backward 2.99 -> 2.83 ms, results bit-identical
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-ffp-contract=off", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function"]


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def build(force=False, verbose=True):
    """All five libraries; returns the core library's path."""
    _build_library(BOX_SOURCES, BOX_HEADERS, BOX_OUT, force, verbose)
    _build_library(GEO_SOURCES, GEO_HEADERS, GEO_OUT, force, verbose)
    _build_library(EXT_SOURCES, EXT_HEADERS, EXT_OUT, force, verbose)
    _build_library(REG_SOURCES, REG_HEADERS, REG_OUT, force, verbose)
    return _build_library(SOURCES, HEADERS, OUT, force, verbose)


def _build_library(sources, headers, out, force, verbose):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.normpath(os.path.join(CSRC, h)) for h in headers]
    jobs = []
    for s in sources:
        src, obj = os.path.join(CSRC, s), os.path.join(objdir, s.replace(".hip", ".o"))
        if force or _newer(src, obj) or any(_newer(h, obj) for h in hdrs):
            jobs.append((src, obj))

    def cc(job):
        src, obj = job
        cmd = [hipcc] + FLAGS + FILE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        return src, r.returncode, r.stdout + r.stderr

    with ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as ex:
        for src, rc, log in ex.map(cc, jobs):
            if verbose and log.strip():
                print(log)
            if rc != 0:
                raise RuntimeError(f"hipcc failed on {src}\n{log}")
            if verbose:
                print(f"[mc_nerf_amd.build] compiled {os.path.basename(src)}")
    objs = [os.path.join(objdir, s.replace(".hip", ".o")) for s in sources]
    if jobs or not os.path.exists(out):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed\n" + r.stdout + r.stderr)
        if verbose:
            print(f"[mc_nerf_amd.build] linked {out}")
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv)
