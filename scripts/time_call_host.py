"""Host time of `call` in the binding of the tree it is run from: entry points that return at N = 0 before any HIP call (null
pointers, no tensors, no GPU), so what is timed is the binding's own work and the ctypes call.

    cd <tree> && python scripts/time_call_host.py [calls per entry point]      -> one line: us per call of each entry point

For an A/B, alternate fresh processes of the two trees (profiles/libraries_once_ab.txt).
"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
from mc_nerf_amd import _geo, _lib, _reg

CASES = ((_lib, "mcnerf_composite_fwd", (None, None, None, 0, None, None, None, 0, 8, 1, None, None, None, None, None, 0)),
         (_reg, "mcnerf_reg_distortion_fwd", (None, None, 0, None, None, 0, 8, 1.0, 0.125, None, None, 0)),
         (_geo, "mcnerf_geo_depth_fwd", (None, None, 0, None, None, 0, 8, None, 0)))
n = int(sys.argv[1]) if len(sys.argv) > 1 else 300000
out = []
for module, name, args in CASES:
    module.call(name, *args)                     # opens the library
    t0 = time.perf_counter()
    for _ in range(n):
        module.call(name, *args)
    out.append(f"{name} {(time.perf_counter() - t0) / n * 1e6:.4f}")
print("  ".join(out))
