"""ctypes binding of libmcnreg.so, the regulariser library (include/mcnerf_reg.h): the entry points of the distortion loss
(DESIGN.md 4i).  Opened on the first `call` only; a missing library raises, there is NO fallback."""
from ._lib import Binding, McnerfError

_B = Binding("mcnerf_reg.h", "libmcnreg.so", "MCNREG_LIB", "mcnerf_reg", "regulariser library")
LIB_PATH, PARAMS, DEFINES, SIGNATURES, ABI_VERSION, lib, loaded, call = _B.LIB_PATH, _B.PARAMS, _B.DEFINES, _B.SIGNATURES, _B.ABI_VERSION, _B.lib, _B.loaded, _B.call
