"""ctypes binding of libmcnhit.so, the hit library (include/mcnerf_hit.h): the entry points that skip the rays missing the scene box
(DESIGN.md 4l).  Opened on the first `call` only; a missing library raises, there is NO fallback."""
from ._lib import Binding, McnerfError

_B = Binding("mcnerf_hit.h", "libmcnhit.so", "MCNHIT_LIB", "mcnerf_hit", "hit library")
LIB_PATH, PARAMS, DEFINES, SIGNATURES, ABI_VERSION, lib, loaded, call = _B.LIB_PATH, _B.PARAMS, _B.DEFINES, _B.SIGNATURES, _B.ABI_VERSION, _B.lib, _B.loaded, _B.call
