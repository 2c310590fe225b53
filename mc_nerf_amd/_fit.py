"""ctypes binding of libmcnfit.so, the fit library (include/mcnerf_fit.h): the entry points that fit the scene box to the voxel sigma
cache.  Opened on the first `call` only; a missing library raises, there is NO fallback."""
from ._lib import Binding, McnerfError

_B = Binding("mcnerf_fit.h", "libmcnfit.so", "MCNFIT_LIB", "mcnerf_fit", "fit library")
LIB_PATH, PARAMS, DEFINES, SIGNATURES, ABI_VERSION, lib, loaded, call = _B.LIB_PATH, _B.PARAMS, _B.DEFINES, _B.SIGNATURES, _B.ABI_VERSION, _B.lib, _B.loaded, _B.call
