"""Builds mc_nerf_amd/libmcnerf.so and, beside it, the libraries of the opt-in features (LIBRARIES and EXTRA_LIBRARIES below; hipcc, gfx950 only) in-tree.

    python -m mc_nerf_amd.build [--force]

hipcc cross-compiles without a GPU; the .so travels to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
_INC = os.path.join("..", "..", "include")
# One entry per library, in build order: prefix of its module attributes -> (.so, sources, what a change of recompiles them).  The
# libraries share the object directory; none links an object of another.  Every list names mcnerf_api.h, the preamble of the
# library's *_api.hip, and mcnerf_multicam.h, which that includes.  A new library is one more entry (the recipe).
LIBRARIES = {
    # skipping the rays that miss the scene box (include/mcnerf_hit.h).  ray_skip.hip includes ray_bounds.hip, and with it
    # select.hip and voxel.hip (listed with the headers: a change of one recompiles ray_skip.hip)
    "HIT_": ("libmcnhit.so", ["hit_api.hip", "ray_skip.hip"],
             ["mcnerf_api.h", "mcnerf_common.h", "mcnerf_kernels.h", "mcnerf_wave.h", "mcnerf_voxel.h", "voxel.hip", "select.hip", "ray_bounds.hip", "mcnerf_compact.h",
              "mcnerf_maxkey.h", "mcnerf_hash.h", "mcnerf_sample_pdf.h", "mcnerf_multicam.h", "mcnerf_ray_bounds.h", "mcnerf_ray_skip.h", os.path.join(_INC, "mcnerf.h"),
              os.path.join(_INC, "mcnerf_hit.h")]),
    # per-ray sample bounds (include/mcnerf_box.h).  The sampler's device code reaches it through mcnerf_sample_pdf.h, the
    # voxel kernels and the lists' scan by ray_bounds.hip including voxel.hip and select.hip (listed with the headers: a change of one
    # recompiles ray_bounds.hip)
    "BOX_": ("libmcnbox.so", ["box_api.hip", "ray_bounds.hip"],
             ["mcnerf_api.h", "mcnerf_common.h", "mcnerf_kernels.h", "mcnerf_wave.h", "mcnerf_voxel.h", "voxel.hip", "select.hip", "mcnerf_compact.h", "mcnerf_maxkey.h",
              "mcnerf_hash.h", "mcnerf_sample_pdf.h", "mcnerf_multicam.h", "mcnerf_ray_bounds.h", os.path.join(_INC, "mcnerf.h"), os.path.join(_INC, "mcnerf_box.h")]),
    # depth supervision (include/mcnerf_geo.h)
    "GEO_": ("libmcngeo.so", ["geo_api.hip", "depth.hip"],
             ["mcnerf_api.h", "mcnerf_common.h", "mcnerf_wave.h", "mcnerf_composite.h", "mcnerf_multicam.h", "mcnerf_depth.h", os.path.join(_INC, "mcnerf.h"),
              os.path.join(_INC, "mcnerf_geo.h")]),
    # alpha-mask supervision (include/mcnerf_ext.h): the first library beside the core, whose ABI is frozen
    "EXT_": ("libmcnext.so", ["ext_api.hip", "mask.hip"],
             ["mcnerf_api.h", "mcnerf_common.h", "mcnerf_wave.h", "mcnerf_composite.h", "mcnerf_multicam.h", "mcnerf_mask.h", os.path.join(_INC, "mcnerf.h"),
              os.path.join(_INC, "mcnerf_ext.h")]),
    # the distortion loss (include/mcnerf_reg.h)
    "REG_": ("libmcnreg.so", ["reg_api.hip", "distortion.hip"],
             ["mcnerf_api.h", "mcnerf_common.h", "mcnerf_wave.h", "mcnerf_composite.h", "mcnerf_multicam.h", "mcnerf_distortion.h", os.path.join(_INC, "mcnerf_reg.h")]),
    # the core library (include/mcnerf.h), last: build() returns its path
    "": ("libmcnerf.so",
         ["api.hip", "pack.hip", "mlp_fwd.hip", "mlp_bwd.hip", "mlp_dw.hip", "pack16.hip", "mlp16_fwd.hip", "mlp16_bwd.hip", "mlp16_dw.hip", "mlp_x3_fwd.hip", "mlp_x3_bwd.hip", "mlp_x3_dw.hip", "composite.hip", "sample_pdf.hip", "select.hip", "rays.hip", "voxel.hip", "optim.hip", "optim_rows.hip", "camera.hip", "color_calib.hip", "errmap.hip", "lens.hip"],
         ["mcnerf_api.h", "mcnerf_common.h", "mcnerf_kernels.h", "mcnerf_wave.h", "mcnerf_composite.h", "mcnerf_16.h", "mcnerf_x3.h", "mcnerf_launch.h", "mcnerf_voxel.h",
          "mcnerf_sample_pdf.h", "mcnerf_multicam.h", "mcnerf_colorcal.h", "mcnerf_errmap.h", "mcnerf_maxkey.h", "mcnerf_compact.h", "mcnerf_hash.h", "mcnerf_rays.h", "mcnerf_lens.h", "mcnerf_optim_rows.h", os.path.join(_INC, "mcnerf.h")]),
}
# The libraries added since that table's length was pinned, in the same shape and in build order: build() makes them ahead of LIBRARIES,
# so the core library is still the last one built.  A library from now on is one more entry HERE.
EXTRA_LIBRARIES = {
    # the scene box fitted to the voxel sigma cache (include/mcnerf_fit.h).  scene_fit.hip includes ray_bounds.hip, and with it
    # select.hip and voxel.hip (listed with the headers: a change of one recompiles scene_fit.hip)
    "FIT_": ("libmcnfit.so", ["fit_api.hip", "scene_fit.hip"],
             ["mcnerf_api.h", "mcnerf_common.h", "mcnerf_kernels.h", "mcnerf_wave.h", "mcnerf_voxel.h", "voxel.hip", "select.hip", "ray_bounds.hip", "mcnerf_compact.h",
              "mcnerf_maxkey.h", "mcnerf_hash.h", "mcnerf_sample_pdf.h", "mcnerf_multicam.h", "mcnerf_ray_bounds.h", "mcnerf_scene_fit.h", os.path.join(_INC, "mcnerf.h"),
              os.path.join(_INC, "mcnerf_fit.h")]),
}
# OUT, SOURCES, HEADERS of the core library and EXT_OUT, EXT_SOURCES, EXT_HEADERS, REG_*, GEO_*, BOX_*, HIT_*, FIT_* of the others
for _prefix, (_so, _sources, _headers) in {**EXTRA_LIBRARIES, **LIBRARIES}.items():
    globals().update({_prefix + "OUT": os.path.join(HERE, _so), _prefix + "SOURCES": _sources, _prefix + "HEADERS": _headers})
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
    """Every library of EXTRA_LIBRARIES and then of LIBRARIES, in their order; returns the core library's path."""
    for so, sources, headers in [*EXTRA_LIBRARIES.values(), *LIBRARIES.values()]:
        out = _build_library(sources, headers, os.path.join(HERE, so), force, verbose)
    return out


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
