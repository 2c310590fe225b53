"""ctypes binding of libmcnbox.so, the bounds library beside libmcnerf.so, libmcnext.so, libmcnreg.so and libmcnbox.so, DERIVED from
include/mcnerf_box.h.

The core ABI (include/mcnerf.h), the extension ABI (include/mcnerf_ext.h), the regulariser ABI (include/mcnerf_reg.h) and the geometry ABI
(include/mcnerf_box.h) are all frozen; the entry points of per-ray sample bounds are here.  As `_ext`: the header is parsed at import with `_lib.parse_header` and checked with `_lib`'s tensor
converters; the LIBRARY is loaded on the first `call` only, so a run that never sets the feature's key never opens it.  There is NO
fallback: a missing library raises.
"""
import ctypes
import os

import torch      # (first, as in _lib: the library's HIP runtime must be torch's)

from . import _lib
from ._lib import McnerfError

_HERE = os.path.dirname(os.path.abspath(__file__))
# MCNBOX_LIB selects another build of the same ABI (as MCNERF_LIB for the core library)
LIB_PATH = os.environ.get("MCNBOX_LIB") or os.path.join(_HERE, "libmcnbox.so")

with open(os.path.join(_HERE, "..", "include", "mcnerf_box.h")) as _f:
    PARAMS, DEFINES = _lib.parse_header(_f.read())
SIGNATURES = {name: (res, [p[2] for p in params]) for name, (res, params) in PARAMS.items()}
ABI_VERSION = DEFINES["MCNERF_BOX_ABI_VERSION"]
_CONVERTERS = {name: tuple(cls and _lib._pointer(name, pname, ctype, cls) for pname, ctype, _, cls in params) for name, (_, params) in PARAMS.items()}
_box = None


def lib():
    """Returns the loaded bounds library; raises McnerfError if it is missing (``python -m mc_nerf_amd.build`` builds all five)."""
    global _box
    if _box is not None:
        return _box
    if not os.path.exists(LIB_PATH):
        raise McnerfError(f"{LIB_PATH} not found: the HIP bounds library is required (python -m mc_nerf_amd.build); there is no CPU fallback")
    try:
        l = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise McnerfError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        if not hasattr(l, name):
            raise McnerfError(f"{LIB_PATH} does not export {name}")
        getattr(l, name).restype, getattr(l, name).argtypes = res, args
    if l.mcnerf_box_abi_version() != ABI_VERSION:
        raise McnerfError("libmcnbox.so ABI version mismatch; rebuild")
    _box = l
    return l


def loaded() -> bool:
    return _box is not None


def call(name, *args):
    """`_lib.call` for an entry point of the bounds library: tensor arguments are checked against the header first (a host tensor
    is refused before the library is opened), a failure raises with the library's message."""
    args = [c(a) if c and isinstance(a, torch.Tensor) else a for c, a in zip(_CONVERTERS[name], args, strict=True)]
    l = lib()
    rc = getattr(l, name)(*args)
    if rc != 0:
        raise McnerfError(f"{name} failed ({rc}): {l.mcnerf_box_last_error().decode()}")
