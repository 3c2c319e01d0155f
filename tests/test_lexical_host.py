"""Host-side checks of the lexical transfer: the CLI surface against the reference's dataclass, the ABI additions, and the
refusal of CPU tensors.  No GPU."""
import ctypes as C
import dataclasses
import os
import re

import pytest
import torch

from zett_amd import _lib
from zett_amd.build import CSRC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zett_lexical_create", "zett_lexical_destroy", "zett_lexical_plan", "zett_lexical_rows_into")


def _header():
    with open(f"{CSRC}/../../include/zett_hip.h") as f:
        return f.read()


def test_cli_fields_and_defaults_are_the_reference_dataclass():
    """scripts/transfer_lexical.py:13-21 of the reference."""
    from zett_amd.lexical import Args
    fields = [(f.name, f.type if isinstance(f.type, str) else f.type.__name__,
               None if f.default is dataclasses.MISSING else f.default) for f in dataclasses.fields(Args)]
    assert fields == [("output", "str", None), ("tokenizer_name", "str", None),
                      ("model_name_or_path", "str", "FacebookAI/xlm-roberta-base"), ("model_class", "str", "AutoModelForMaskedLM"),
                      ("fvt_mode", "str", "no"), ("fallback_mode", "str", "unk"), ("save_flax", "bool", False)]


def test_cli_shim_points_at_the_package():
    with open(os.path.join(REPO, "scripts", "transfer_lexical.py")) as f:
        assert "from zett_amd.lexical import main" in f.read()


def test_symbols_in_header_binding_and_library():
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = _lib.load()
    assert lib.zett_abi_version() == 8 and re.search(r"#define ZETT_ABI_VERSION 8\b", header)
    for name in NEW:
        assert name in _lib.ABI_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        getattr(lib, name)


@pytest.mark.parametrize("name", NEW)
def test_argtypes_match_the_header(name):
    """Every parameter of the declaration against the ctypes binding: pointers are void* / POINTER, integers by width."""
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    params = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header, re.S).group(1)
    fn = getattr(_lib.load(), name)
    want = []
    for p in (q.strip() for q in params.split(",")):
        if "*" in p:
            want.append("ptr")
        elif p.startswith("int64_t"):
            want.append(C.c_int64)
        elif p.startswith("int32_t"):
            want.append(C.c_int32)
        elif p.startswith("int "):
            want.append(C.c_int)
        else:
            raise AssertionError(p)
    assert len(fn.argtypes) == len(want), (name, len(fn.argtypes), len(want))
    for i, (have, w) in enumerate(zip(fn.argtypes, want)):
        if w == "ptr":
            assert have is C.c_void_p or issubclass(have, C._Pointer), (name, i, have)
        else:
            assert C.sizeof(have) == C.sizeof(w) and have(-1).value == -1, (name, i, have)


def test_mode_constants_match_the_header():
    m = re.search(r"enum zett_lexical_mode \{(.*?)\}", _header(), re.S).group(1)
    values = {k: int(v) for k, v in re.findall(r"(ZETT_LEXICAL_\w+)\s*=\s*(\d+)", m)}
    assert values == {"ZETT_LEXICAL_NO": _lib.LEXICAL_NO, "ZETT_LEXICAL_FVT": _lib.LEXICAL_FVT, "ZETT_LEXICAL_BFVT": _lib.LEXICAL_BFVT}
    from zett_amd.lexical import FVT_MODES
    assert FVT_MODES == {"no": 0, "fvt": 1, "bfvt": 2}


def test_bad_arguments_refused_before_the_device():
    lib = _lib.load()
    d = _lib.ZettDest()
    assert lib.zett_lexical_create(None, 0, None, None, None, 0, None) == _lib.E_INVALID
    assert lib.zett_lexical_plan(None, None, 1, 0, 1, 0, 1, None, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.zett_lexical_rows_into(None, None, None, 1, 1, None, 1, None, 1, 0, 1, 1, -1, C.byref(d), None) == _lib.E_INVALID
    assert lib.zett_lexical_destroy(None) == 0


def test_cpu_is_refused():
    from zett_amd import lexical
    with pytest.raises(RuntimeError, match="MI355X"):
        lexical.LexicalTransfer(object(), "cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        lexical.lexical_embeddings(object(), ["a"], torch.zeros(4, 8))
    plan = lexical.LexicalPlan(torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0, 0, 4, "no")
    lt = lexical.LexicalTransfer.__new__(lexical.LexicalTransfer)
    with pytest.raises(RuntimeError, match="MI355X"):
        lt.rows_into(plan, torch.zeros(4, 8), dest_in=torch.zeros(1, 8))


def test_save_flax_and_missing_unk_are_clear_errors():
    from zett_amd import lexical
    with pytest.raises(NotImplementedError, match="Flax"):
        lexical.main(["--output", "o", "--tokenizer_name", "t", "--save_flax", "true"])
    with pytest.raises(ValueError, match="fvt_mode"):
        lexical.main(["--output", "o", "--tokenizer_name", "t", "--fvt_mode", "sometimes"])


def test_product_module_does_not_import_the_oracle():
    with open(os.path.join(REPO, "zett_amd", "lexical.py")) as f:
        src = f.read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", src, re.M)


def test_division_is_not_a_reciprocal_multiply():
    """The mean's one division must be IEEE: the build has no fast-math flag (zett_amd/build.py)."""
    from zett_amd.build import HIPCC_FLAGS
    assert not any("fast-math" in f or "unsafe-fp" in f or "correctly-rounded" in f for f in HIPCC_FLAGS)
