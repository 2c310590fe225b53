"""ctypes binding of libmcnext.so, the extension library (include/mcnerf_ext.h): the entry points of alpha-mask supervision
(DESIGN.md 4h).  Opened on the first `call` only; a missing library raises, there is NO fallback."""
from ._lib import Binding, McnerfError

_B = Binding("mcnerf_ext.h", "libmcnext.so", "MCNEXT_LIB", "mcnerf_ext", "extension library")
LIB_PATH, PARAMS, DEFINES, SIGNATURES, ABI_VERSION, lib, loaded, call = _B.LIB_PATH, _B.PARAMS, _B.DEFINES, _B.SIGNATURES, _B.ABI_VERSION, _B.lib, _B.loaded, _B.call
