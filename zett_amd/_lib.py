"""ctypes binding of libzett_hip.so, read from its C ABI: include/zett_hip.h is the only declaration of an entry point, a constant or a
struct, and this module binds what zett_amd/_header.py finds there.

The library is the product: if it cannot be loaded there is no fallback — the import of anything that computes raises.

Constants: ZETT_X of the header is X here (E_INVALID, RANGE_DEST, MT_CHUNK, ABI_VERSION ...), available without the library; ZETT_OK and
DTYPE_F32 / DTYPE_F16 / DTYPE_BF16 are the written-out exceptions, ENCODE_MAX_ADDED / ENCODE_MAX_ADDED_BYTES the two limits the header only describes.  ABI_SYMBOLS: the declared functions, in header order.
Structs: zett_fwd_gemm_desc is the ctypes.Structure ZettFwdGemmDesc, field for field; a field named like a Python keyword gains an
underscore (zett_dest.in is ZettDest.in_).
Types, for parameters, return values and fields alike:
    int c_int | int32_t c_int32 | int64_t c_int64 | uint64_t c_uint64 | float c_float | double c_double | const char* c_char_p
    a pointer to one of the structs: POINTER(that Structure);  every other pointer: c_void_p — the header cannot tell a device pointer
    from a host out-parameter, and c_void_p takes byref(...), ctypes arrays, None and c_void_p values alike.
The reader is strict: a line of the header's extern "C" part outside the forms and types it knows (zett_amd/_header.py lists them) is a
HeaderError on import that names the line, never a declaration passed over or a guessed prototype.
"""
from __future__ import annotations

import ctypes as C
import keyword
import os
import threading

from . import _header
from .build import LIB_PATH

_H = _header.read()
globals().update({name.removeprefix("ZETT_"): value for name, value in _H.constants.items()})
ZETT_OK = _H.constants["ZETT_OK"]
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = (_H.constants[n] for n in ("ZETT_F32", "ZETT_F16", "ZETT_BF16"))
ENCODE_MAX_ADDED, ENCODE_MAX_ADDED_BYTES = 512, 64      # zett_encode_texts_added: tokens of a table, bytes of a token (the header states them in prose only)
ABI_SYMBOLS = tuple(_H.functions)

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double,
            "const char*": C.c_char_p}
_STRUCTS = {}      # "zett_dest" -> ZettDest


def _ctype(c_type: str):
    if c_type in _SCALARS:
        return _SCALARS[c_type]
    pointee = c_type.replace("const ", "")[:-1]      # a struct's name when c_type is one pointer to a struct
    return C.POINTER(_STRUCTS[pointee]) if pointee in _STRUCTS else C.c_void_p


for _name, _fields in _H.structs.items():
    _cls = type("".join(w.capitalize() for w in _name.split("_")), (C.Structure,), {
        "__doc__": f"struct {_name} of include/zett_hip.h",
        "_fields_": [(f + "_" if keyword.iskeyword(f) else f, _ctype(t)) for f, t in _fields]})
    _STRUCTS[_name] = globals()[_cls.__name__] = _cls
del _name, _fields, _cls


_lib = None
_lock = threading.Lock()


def lib_path() -> str:
    return os.environ.get("ZETT_HIP_LIB", LIB_PATH)


def load():
    """dlopen the library (once) and declare the header's prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: the HIP extension has not been built. Run "
                "`python -m zett_amd.build` (needs hipcc); zett_amd has no CPU fallback.")
        lib = C.CDLL(path)
        for name, (result, params) in _H.functions.items():
            if not hasattr(lib, name):
                raise RuntimeError(f"{path} does not export {name}, which include/zett_hip.h declares: rebuild it (`python -m zett_amd.build`)")
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _ctype(result), [_ctype(p) for p in params]
        if lib.zett_abi_version() != ABI_VERSION:      # the header this package reads is that version's
            raise RuntimeError(f"{path} has ABI version {lib.zett_abi_version()}, this package expects {ABI_VERSION}: "
                               "rebuild it (`python -m zett_amd.build`)")
        _lib = lib
    return _lib


class RangeError(OverflowError):
    """ZETT_E_RANGE: a value left the range of the 16-bit operand type, or an output is not finite."""


def check(rc: int, what: str = "") -> None:
    """Map a negative status to the exception the reference would raise."""
    if rc == ZETT_OK:
        return
    msg = load().zett_last_error().decode("utf-8", "replace")
    if what:
        msg = f"{what}: {msg}"
    if rc == E_INDEX:
        raise IndexError(msg)
    if rc == E_NOT_IMPLEMENTED:
        raise NotImplementedError(msg)
    if rc == E_KEY:
        raise KeyError(msg)
    if rc == E_INVALID:
        raise ValueError(msg)
    if rc == E_RANGE:
        raise RangeError(msg)
    raise RuntimeError(msg)
