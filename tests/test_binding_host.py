"""The whole boundary in one place (no GPU): include/zett_hip.h is the only declaration of the C ABI, zett_amd/_header.py reads it and
zett_amd/_lib.py binds what was read.  Three checks: the reader on small snippets (what it accepts, and that it refuses everything else
with the line); the host compiler as an independent judge of every constant, struct layout and prototype the binding declares; and the
functions the built library exports against the ones the header declares."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

from zett_amd import _header, _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reader, on snippets --------------------------------------------------------------------------------------------------------
def test_reader_accepts_the_forms_the_header_uses():
    h = _header.parse("""
        #define ZETT_N 65536      /* a comment; with (punctuation) and the word int */
        // another; one (here)
        enum zett_e { ZETT_A = 0, ZETT_B = -7 };
        enum zett_bits {
            ZETT_ONE = 1,      /* first; */
            ZETT_TWO = 2
        };
        typedef struct zett_h zett_h;
        typedef struct zett_rec {
            int32_t m, n, k;              /* int32_t x; */
            void* in; void* out;
            const int64_t* rows;
            double d; float f; int64_t big; uint64_t u; int i;
        } zett_rec;
        const char* zett_last_error(void);
        int zett_make(const zett_rec* rec, int device, zett_h** out);
        int zett_use(const zett_h* h, const void* const* list, void* const* outs, const char* key, uint32_t* counts,
                     float scale, double eps, uint64_t seed, const uint8_t* mask, void* stream);
    """)
    assert h.constants == {"ZETT_N": 65536, "ZETT_A": 0, "ZETT_B": -7, "ZETT_ONE": 1, "ZETT_TWO": 2}
    assert list(h.structs) == ["zett_rec"] and h.structs["zett_rec"] == [
        ("m", "int32_t"), ("n", "int32_t"), ("k", "int32_t"), ("in", "void*"), ("out", "void*"), ("rows", "const int64_t*"),
        ("d", "double"), ("f", "float"), ("big", "int64_t"), ("u", "uint64_t"), ("i", "int")]
    assert list(h.functions) == ["zett_last_error", "zett_make", "zett_use"]
    assert h.functions["zett_last_error"] == ("const char*", [])
    assert h.functions["zett_make"] == ("int", ["const zett_rec*", "int", "zett_h**"])
    assert h.functions["zett_use"] == ("int", ["const zett_h*", "const void* const*", "void* const*", "const char*", "uint32_t*", "float", "double",
                                               "uint64_t", "const uint8_t*", "void*"])


def test_reader_reads_only_the_extern_c_part():
    h = _header.parse('#ifndef X_H\n#define X_H\n#include <stdint.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n#define ZETT_V 3\nint zett_f(void);\n'
                      "#ifdef __cplusplus\n}\n#endif\n#endif /* X_H */\n")
    assert h.constants == {"ZETT_V": 3} and list(h.functions) == ["zett_f"]
    with pytest.raises(_header.HeaderError, match=r":4: .*never closed"):
        _header.parse('#define ZETT_V 3\n\n\n#ifdef __cplusplus\nextern "C" {\n#endif\nint zett_f(void);\n')


REFUSED = [      # (text, the line that must be named)
    ("enum zett_e {\n  ZETT_A = 0,\n  ZETT_B\n};", 3),                                   # an enumerator without a value
    ("enum zett_e { ZETT_A = 1 << 2 };", 1),                                              # values that are no decimal integer literal
    ("enum zett_e {\n  ZETT_A = 1,\n  ZETT_B = ZETT_A\n};", 3),
    ("\n#define ZETT_X (3)", 2),
    ("#define ZETT_X 0x10", 1),
    ("#define ZETT_X 3u", 1),
    ("#define ZETT_X 1\n#define ZETT_Y ZETT_X", 2),
    ("#define ZETT_F(x) 3", 1),
    ("#include <stdio.h>", 1),
    ("int zett_f(int32_t a,\n           long n);", 2),                                    # types outside the table
    ("typedef struct zett_s {\n  int32_t a;\n  unsigned b;\n} zett_s;", 3),
    ("int zett_f(int16_t* p);", 1),
    ("int zett_f(char* s);", 1),
    ("int zett_f(const int32_t n);", 1),
    ("int zett_f(zett_undeclared* h);", 1),
    ("\nvoid zett_f(int a);", 2),
    ("typedef struct zett_s {\n  int32_t a;\n  int (*cb)(int);\n} zett_s;", 3),           # function-pointer, array and bit-field members
    ("typedef struct zett_s {\n  float v[4];\n} zett_s;", 2),
    ("typedef struct zett_s {\n  int32_t a : 3;\n} zett_s;", 2),
    ("typedef struct zett_s {\n  int32_t *a, *b;\n} zett_s;", 2),
    ("typedef struct zett_s {\n  int32_t a;\n  struct { int32_t b; } inner;\n} zett_s;", 1),
    ("int zett_ok(void);\nint zett_f(int (*cb)(int));", 2),                               # declarations of a form the reader does not know
    ("int zett_f(int a, ...);", 1),
    ("int zett_f(int);", 1),
    ("\n\nstatic inline int zett_f(void) { return 0; }", 3),
    ("union zett_u { int a; };", 1),
    ("extern int zett_counter;", 1),
    ("typedef int32_t zett_id;", 1),
    ("typedef struct zett_s { int32_t a; } zett_t;", 1),
    ("int zett_f(void);\n\nint zett_g(int a)", 3),
    ("#define ZETT_X 1\nenum zett_e { ZETT_X = 1 };", 2),                                  # declared twice
    ("int zett_f(void);\nint zett_f(int a);", 2),
]


@pytest.mark.parametrize("text,line", REFUSED, ids=[re.sub(r"\s+", " ", t)[:40] for t, _ in REFUSED])
def test_reader_refuses_what_it_does_not_understand_and_names_the_line(text, line):
    with pytest.raises(_header.HeaderError, match=rf"^snippet\.h:{line}: "):
        _header.parse(text, "snippet.h")


# ---- the compiler agrees with the reader, and the binding with the compiler ----------------------------------------------------------
PROGRAM = """\
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "zett_hip.h"
template <class T> void traits() {      // size, pointer, floating point, signed
    std::printf(" %zu:%d:%d:%d", sizeof(T), int(std::is_pointer<T>::value), int(std::is_floating_point<T>::value), int(std::is_signed<T>::value));
}
template <class F> struct prototype;      // over decltype(&zett_name): no type is named by hand and no function is referenced
template <class R, class... A> struct prototype<R (*)(A...)> {
    static void print(const char* name) {
        std::printf("F %s %zu", name, sizeof...(A));
        traits<R>();
        (traits<A>(), ...);
        std::printf("\\n");
    }
};
int main() {
@BODY@    return 0;
}
"""


def _traits(t):
    """what the program prints for a C type, of the ctypes type bound to it"""
    pointer = t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer)
    return f"{C.sizeof(t)}:{int(pointer)}:{int(t in (C.c_float, C.c_double))}:{int(not pointer and t(-1).value == -1)}"


@pytest.fixture(scope="module")
def judged(tmp_path_factory):
    """The lines a C++17 program prints about everything the reader found in include/zett_hip.h: compiled for the host alone by the
    toolchain that builds the library, linked against nothing of ours, run here."""
    h = _header.read()
    body = [f'    std::printf("C {n} %lld\\n", (long long){n});\n' for n in h.constants]
    for s, fields in h.structs.items():
        body.append(f'    std::printf("S {s} %zu", sizeof({s}));\n')
        for f, _ in fields:
            body.append(f'    std::printf(" {f}@%zu", offsetof({s}, {f})); traits<decltype({s}::{f})>();\n')
        body.append('    std::printf("\\n");\n')
    body += [f'    prototype<decltype(&{n})>::print("{n}");\n' for n in h.functions]
    work = tmp_path_factory.mktemp("binding")
    source, program = work / "judge.cpp", work / "judge"
    source.write_text(PROGRAM.replace("@BODY@", "".join(body)))
    subprocess.run([build._hipcc(), "-x", "c++", "-no-hip-rt", "-std=c++17", "-O0", "-I", os.path.join(REPO, "include"), str(source), "-o", str(program)],
                   check=True, timeout=300)
    lines = subprocess.run([str(program)], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    return {kind: [l.split()[1:] for l in lines if l.startswith(kind + " ")] for kind in "CSF"}


def test_constants_have_the_compilers_values(judged):
    h = _header.read()
    seen = {name: int(value) for name, value in judged["C"]}
    assert seen == h.constants and len(seen) >= 80
    # nothing was passed over: every ZETT_ identifier in the header's code (comments removed) is one of them
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(_header.PATH).read(), flags=re.S)
    assert set(re.findall(r"\bZETT_[A-Z0-9_]+\b", code)) - {"ZETT_HIP_H"} == set(seen)
    for name, value in seen.items():
        assert getattr(_lib, name[len("ZETT_"):]) == value, name
    assert (_lib.ZETT_OK, _lib.DTYPE_F32, _lib.DTYPE_F16, _lib.DTYPE_BF16) == (seen["ZETT_OK"], seen["ZETT_F32"], seen["ZETT_F16"], seen["ZETT_BF16"])
    assert _lib.ABI_VERSION == seen["ZETT_ABI_VERSION"] == 8
    assert (_lib.E_INVALID, _lib.E_RANGE, _lib.RANGE_DEST, _lib.MT_CHUNK, _lib.LN_WORKGROUP) == (-1, -7, 16, 65536, 3)


def test_structures_have_the_compilers_layout(judged):
    h = _header.read()
    assert [s[0] for s in judged["S"]] == list(h.structs) and len(h.structs) == 7
    names = {"zett_config": "ZettConfig", "zett_stats": "ZettStats", "zett_gemm_record": "ZettGemmRecord", "zett_dest": "ZettDest",
             "zett_fwd_gemm_desc": "ZettFwdGemmDesc", "zett_sampled_vocab_record": "ZettSampledVocabRecord", "zett_retok_model": "ZettRetokModel"}
    for name, size, *fields in judged["S"]:
        cls = getattr(_lib, names[name])
        assert issubclass(cls, C.Structure) and C.sizeof(cls) == int(size), name
        assert len(fields) == 2 * len(cls._fields_) == 2 * len(h.structs[name]), name
        for (py_name, ctype), (c_name, _), at, traits in zip(cls._fields_, h.structs[name], fields[0::2], fields[1::2]):
            assert py_name == (c_name + "_" if c_name == "in" else c_name), (name, c_name)
            assert at == f"{c_name}@{getattr(cls, py_name).offset}" and traits == _traits(ctype), (name, c_name, at, traits)
    assert _lib.ZettDest.in_.offset == 0 and _lib.ZettDest.rows.offset == 48 and C.sizeof(_lib.ZettFwdGemmDesc) == 264


def test_prototypes_have_the_compilers_types(judged):
    h = _header.read()
    assert [f[0] for f in judged["F"]] == list(h.functions) == list(_lib.ABI_SYMBOLS) and len(h.functions) >= 107
    lib = _lib.load()
    for name, count, result, *params in judged["F"]:
        fn = getattr(lib, name)
        assert int(count) == len(params) == len(fn.argtypes) == len(h.functions[name][1]), name
        assert result == _traits(fn.restype), (name, result, fn.restype)
        assert fn.restype is (C.c_char_p if name == "zett_last_error" else C.c_int), name
        for i, (want, have, spelled) in enumerate(zip(params, fn.argtypes, h.functions[name][1])):
            assert want == _traits(have), (name, i, spelled, want, have)
            if have not in (C.c_void_p, C.c_char_p) and issubclass(have, C._Pointer):      # POINTER(Structure): of the struct the header names
                assert issubclass(have._type_, C.Structure) and spelled.replace("const ", "") == re.sub(r"(?<!^)(?=[A-Z])", "_", have._type_.__name__).lower() + "*", (name, i)
    assert lib.zett_forward_into.argtypes[8] is C.POINTER(_lib.ZettDest) and lib.zett_create.argtypes[0] is C.POINTER(_lib.ZettConfig)
    assert lib.zett_set_option.argtypes == [C.c_void_p, C.c_char_p, C.c_int64]


# ---- header and library agree -------------------------------------------------------------------------------------------------------
def _exported_functions(path):
    """names of the functions an ELF64 shared object defines in its dynamic symbol table"""
    with open(path, "rb") as f:
        elf = f.read()
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, kind, _, _, offset, size, link, _, _, entsize in sections:
        if kind != 11:      # SHT_DYNSYM
            continue
        strings = sections[link][4]
        for at in range(offset, offset + size, entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", elf, at)
            if st_info & 0xF == 2 and st_shndx != 0:      # STT_FUNC, defined here
                names.add(elf[strings + st_name:elf.index(b"\0", strings + st_name)].decode())
    return names


def test_library_exports_exactly_the_declared_functions():
    exported = {n for n in _exported_functions(_lib.lib_path()) if n.startswith("zett_")}
    assert exported == set(_header.read().functions) == set(_lib.ABI_SYMBOLS), exported ^ set(_lib.ABI_SYMBOLS)
    assert len(_lib.ABI_SYMBOLS) == len(set(_lib.ABI_SYMBOLS))


def test_load_names_a_declared_function_the_library_lacks(tmp_path, monkeypatch):
    """a library without one of the header's functions fails in load(), by name"""
    empty = tmp_path / "libempty.so"
    subprocess.run([build._hipcc(), "-x", "c++", "-no-hip-rt", "-shared", "-fPIC", "-o", str(empty), os.devnull], check=True, timeout=300)
    monkeypatch.setattr(_lib, "_lib", None)      # load() binds once per process: as if it had not yet
    monkeypatch.setenv("ZETT_HIP_LIB", str(empty))
    with pytest.raises(RuntimeError, match=r"libempty\.so does not export zett_last_error, which include/zett_hip\.h declares"):
        _lib.load()
    assert _lib._lib is None
