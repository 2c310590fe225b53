"""ctypes binding of libmcngeo.so, the geometry library (include/mcnerf_geo.h): the entry points of depth supervision
(DESIGN.md 4j).  Opened on the first `call` only; a missing library raises, there is NO fallback."""
from ._lib import Binding, McnerfError

_B = Binding("mcnerf_geo.h", "libmcngeo.so", "MCNGEO_LIB", "mcnerf_geo", "geometry library")
LIB_PATH, PARAMS, DEFINES, SIGNATURES, ABI_VERSION, lib, loaded, call = _B.LIB_PATH, _B.PARAMS, _B.DEFINES, _B.SIGNATURES, _B.ABI_VERSION, _B.lib, _B.loaded, _B.call
