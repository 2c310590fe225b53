"""ctypes binding of libmcnbox.so, the bounds library (include/mcnerf_box.h): the entry points of per-ray sample bounds
(DESIGN.md 4k).  Opened on the first `call` only; a missing library raises, there is NO fallback."""
from ._lib import Binding, McnerfError

_B = Binding("mcnerf_box.h", "libmcnbox.so", "MCNBOX_LIB", "mcnerf_box", "bounds library")
LIB_PATH, PARAMS, DEFINES, SIGNATURES, ABI_VERSION, lib, loaded, call = _B.LIB_PATH, _B.PARAMS, _B.DEFINES, _B.SIGNATURES, _B.ABI_VERSION, _B.lib, _B.loaded, _B.call
