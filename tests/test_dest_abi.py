"""CPU checks of the destination-store ABI (include/zett_hip.h zett_forward_into): exported symbols, the layout of struct
zett_dest as the ctypes binding declares it, the new range bit, and argument validation that happens before any launch."""
import ctypes as C
import re

from zett_amd import _lib
from zett_amd.build import CSRC


def test_symbols_exported():
    lib = _lib.load()
    for name in ("zett_forward_into", "zett_forward_table_into"):
        assert name in _lib.ABI_SYMBOLS
        getattr(lib, name)
    assert lib.zett_abi_version() == 8


def test_dest_struct_layout_matches_header():
    D = _lib.ZettDest
    assert C.sizeof(D) == 64
    offsets = {name: getattr(D, name).offset for name, _ in D._fields_}
    assert offsets == {"in_": 0, "out": 8, "bias": 16, "dtype": 24, "bias_dtype": 28, "ld_in": 32, "ld_out": 40, "rows": 48, "n_dest_rows": 56}
    with open(f"{CSRC}/../../include/zett_hip.h") as f:
        header = f.read()
    body = re.search(r"typedef struct zett_dest \{(.*?)\} zett_dest;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*?\s*(\w+)\s*[;,]", body)
    assert names == ["in", "out", "bias", "dtype", "bias_dtype", "ld_in", "ld_out", "rows", "n_dest_rows"]


def test_range_dest_bit():
    assert _lib.RANGE_DEST == 16
    with open(f"{CSRC}/../../include/zett_hip.h") as f:
        assert re.search(r"ZETT_RANGE_DEST\s*=\s*16", f.read())


def test_bad_arguments_refused_before_the_device():
    lib = _lib.load()
    d = _lib.ZettDest()
    rc = lib.zett_forward_into(None, None, 1, 1, None, 0, 1, -1, C.byref(d), None)
    assert rc == _lib.E_INVALID
    rc = lib.zett_forward_table_into(None, None, 1, 1, None, None, None, -1, C.byref(d), None)
    assert rc == _lib.E_INVALID
