"""ctypes binding of libmcnerf.so, DERIVED from include/mcnerf.h, the one statement of the C ABI, and the `Binding` class that the
libraries beside it (`_ext`, `_reg`, `_geo`, `_box`, `_hit`, `_fit`) are bound with as well.

The header is parsed once at import (`parse_header`): every prototype gives an entry point's ctypes signature (`SIGNATURES`), its
parameter names and, per pointer, the dtype a tensor handed to it must have (`PARAMS`); every decimal `#define MCNERF_*` gives a
constant (`DEFINES`).  A type the parser does not know is an import error that names the prototype: nothing is guessed.

There is deliberately NO fallback: if the HIP library is missing or does not load, `lib()` raises and every op in ``mc_nerf_amd.ops`` fails loudly.
"""
import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int, c_longlong, c_void_p

# torch ships its own HIP runtime (torch/lib/libamdhip64.so).  It MUST be in the process before
# libmcnerf.so is loaded, so that the library's libamdhip64 dependency resolves to the same runtime
# instance that owns torch's streams and allocations (two runtimes in one process do not share devices).
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST = "host table"      # element class of a pointer into HOST memory: long long*, T* const*, and what the header marks MCNERF_HOST
BY_VALUE = {"int": c_int, "long long": c_longlong, "float": c_float}
# element type of a pointer -> dtype of the device tensor it takes (the unsigned words travel in signed tensors, void* is bytes)
ELEMENT = {"float": torch.float32, "int32_t": torch.int32, "uint32_t": torch.int32, "int64_t": torch.int64, "uint64_t": torch.int64,
           "uint8_t": torch.uint8, "void": torch.uint8, "long long": HOST}


class McnerfError(RuntimeError):
    pass


def _classify(ctype):
    """C parameter type -> (ctypes type, element class: None by value, a torch dtype, or HOST); raises on any other type."""
    host = ctype.lstrip().startswith("MCNERF_HOST ")
    t = " ".join(re.findall(r"\w+|\S", ctype)).removeprefix("MCNERF_HOST ").removeprefix("const ")
    if not host and t in BY_VALUE:
        return BY_VALUE[t], None
    base, table = re.fullmatch(r"(long long|\w+) \*( const \*)?", t).groups()
    return c_void_p, HOST if ELEMENT[base] is HOST or host or table else ELEMENT[base]


def parse_header(text):
    """Header text -> ({function: (restype, ((parameter name, C type, ctypes type, element class), ...))}, {MCNERF_* define: int})."""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    defines = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MCNERF_\w+)[ \t]+(\d+)[ \t]*$", text, flags=re.M)}
    code = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    functions = {}
    for ret, name, args in re.findall(r"([\w\s*]+?)\b(mcnerf_\w+)\s*\(([^()]*)\)\s*;", code):
        try:
            restype = {"const char *": c_char_p, **BY_VALUE}[" ".join(re.findall(r"\w+|\*", ret))]
            params = []
            for arg in ([] if args.strip() in ("", "void") else args.split(",")):
                ctype, pname = re.fullmatch(r"\s*(.*[\s*])(\w+)\s*", arg, flags=re.S).groups()
                params.append((pname, " ".join(ctype.split()), *_classify(ctype)))
        except (KeyError, AttributeError):
            raise McnerfError(f"include/mcnerf.h: {name}: '{ret.strip()}' or a parameter of ({' '.join(args.split())}) has a type the binding does not know") from None
        functions[name] = (restype, tuple(params))
    unparsed = set(re.findall(r"\b(mcnerf_\w+)\s*\(", code)) - set(functions)
    if unparsed:
        raise McnerfError(f"include/mcnerf.h: cannot parse the prototype of {sorted(unparsed)}")
    return functions, defines


def _pointer(fn, pname, ctype, want):
    """Converter of a tensor at one pointer position -> its checked device address."""
    def conv(a):
        if want is HOST:
            raise McnerfError(f"{fn}: {pname} ({ctype}) is a host array: it takes a ctypes array, not a tensor")
        if not a.is_cuda:
            raise McnerfError(f"{fn}: {pname} must be a CUDA/HIP tensor (no CPU fallback), got one on {a.device}")
        if a.dtype != want:
            raise McnerfError(f"{fn}: {pname} ({ctype}) takes a {want} tensor, got {a.dtype}")
        if not a.is_contiguous():
            raise McnerfError(f"{fn}: {pname} must be contiguous")
        return a.data_ptr()
    return conv


class Binding:
    """One library and the header it is derived from: include/<header> is parsed when the binding is made, mc_nerf_amd/<soname> (or
    the build of the same ABI that the environment variable `env` names, e.g. the parent commit's) is opened by the first `lib()` /
    `call()` only.  `prefix` is that of the library's `<prefix>_abi_version` / `<prefix>_last_error` pair and, in capitals, of its
    `<PREFIX>_ABI_VERSION`; `noun` is what the "not found" text calls the library."""

    def __init__(self, header, soname, env, prefix, noun):
        self.soname, self.prefix, self.noun = soname, prefix, noun
        self.LIB_PATH = os.environ.get(env) or os.path.join(_HERE, soname)
        with open(os.path.join(_HERE, "..", "include", header)) as f:
            self.PARAMS, self.DEFINES = parse_header(f.read())
        self.SIGNATURES = {name: (res, [p[2] for p in params]) for name, (res, params) in self.PARAMS.items()}      # name -> (restype, argtypes)
        self.ABI_VERSION = self.DEFINES[prefix.upper() + "_ABI_VERSION"]
        # per entry point one converter per position (None: by value); whatever is not a tensor goes to ctypes as it is: None (NULL),
        # raw addresses (data_ptr(), the stream), ctypes arrays and casts
        self._converters = {name: tuple(cls and _pointer(name, pname, ctype, cls) for pname, ctype, _, cls in params)
                            for name, (_, params) in self.PARAMS.items()}
        self._lib = None

    def lib(self):
        """Returns the loaded library; raises McnerfError if it is missing (``python -m mc_nerf_amd.build`` builds every library)."""
        if self._lib is not None:
            return self._lib
        if not os.path.exists(self.LIB_PATH):
            raise McnerfError(f"{self.LIB_PATH} not found: the HIP {self.noun} is required (python -m mc_nerf_amd.build); there is no CPU fallback")
        try:
            l = ctypes.CDLL(self.LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise McnerfError(f"cannot load {self.LIB_PATH}: {e}") from e
        for name, (res, args) in self.SIGNATURES.items():
            if not hasattr(l, name):
                raise McnerfError(f"{self.LIB_PATH} does not export {name}")
            getattr(l, name).restype, getattr(l, name).argtypes = res, args
        if getattr(l, self.prefix + "_abi_version")() != self.ABI_VERSION:
            raise McnerfError(f"{self.soname} ABI version mismatch; rebuild")
        self._lib = l
        return l

    def loaded(self) -> bool:
        return self._lib is not None

    def call(self, name, *args):
        """Calls a status-returning entry point and raises with the library's message on failure.  Tensor arguments are first checked
        against the header: a host tensor is refused before the library is opened."""
        args = [c(a) if c and isinstance(a, torch.Tensor) else a for c, a in zip(self._converters[name], args, strict=True)]
        l = self.lib()
        rc = getattr(l, name)(*args)
        if rc != 0:
            raise McnerfError(f"{name} failed ({rc}): {getattr(l, self.prefix + '_last_error')().decode()}")


# libmcnerf.so, the core library (include/mcnerf.h).  There is no fallback: if it is missing or does not load, `lib()` raises
_CORE = Binding("mcnerf.h", "libmcnerf.so", "MCNERF_LIB", "mcnerf", "extension")
LIB_PATH, PARAMS, DEFINES, SIGNATURES, ABI_VERSION = _CORE.LIB_PATH, _CORE.PARAMS, _CORE.DEFINES, _CORE.SIGNATURES, _CORE.ABI_VERSION
lib, loaded, call = _CORE.lib, _CORE.loaded, _CORE.call


