"""What every wrapper needs to pass torch tensors through the C ABI (zett_amd/_lib.py): pointers, stream handles, the dtype codes
and the default device.  torch is imported inside the functions: the modules that import it lazily stay that way.
"""
from __future__ import annotations

import ctypes as C
import functools

from . import _lib


def ptr(t, byte_offset: int = 0) -> C.c_void_p:
    """the address of a tensor's first element (plus ``byte_offset``); null for ``None``"""
    return C.c_void_p(0 if t is None else t.data_ptr() + byte_offset)


def stream(device=None, of=None) -> C.c_void_p:
    """the handle of ``device``'s current stream, or of the torch stream ``of``"""
    import torch
    return C.c_void_p((torch.cuda.current_stream(device) if of is None else of).cuda_stream)


@functools.lru_cache(maxsize=None)
def zett_dtypes() -> dict:
    """torch dtype -> zett_dtype, for the element types the kernels read and write"""
    import torch
    return {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def default_device(device=None):
    """``torch.device(device)``; the current cuda (ROCm) device for ``None``"""
    import torch
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("zett_amd computes on MI355X only: no cuda (ROCm) device is visible; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())
