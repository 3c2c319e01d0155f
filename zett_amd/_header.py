"""Reader of include/zett_hip.h: the header is the only declaration of the C ABI, zett_amd/_lib.py binds what this finds.

Pure Python, standard library only.  The ``extern "C"`` part of the header is a sequence of five forms, and anything else in it is a
HeaderError that names the line — never skipped, so a new form in the header fails on import instead of giving a wrong prototype:

    #define ZETT_X <decimal integer>
    enum zett_x { ZETT_A = <decimal integer>, ... };                 every enumerator with its value
    typedef struct zett_x zett_x;                                    an opaque handle
    typedef struct zett_x { <type> a, b; <type> c; ... } zett_x;     scalar and pointer fields only
    <type> zett_name(<type> name, ...);    or (void)

A <type> is one of SCALARS by value, or a pointer (any depth, const anywhere) to one of POINTEES, a handle or a struct declared above.
"""
from __future__ import annotations

import os
import re
from typing import NamedTuple

from .build import CSRC, HEADERS

PATH = os.path.normpath(os.path.join(CSRC, HEADERS[-1]))      # include/zett_hip.h
SCALARS = ("int", "int32_t", "int64_t", "uint64_t", "float", "double")
POINTEES = ("void", "char", "float", "double", "uint8_t", "int32_t", "uint32_t", "int64_t")

_INT = r"-?(?:0|[1-9][0-9]*)"
_TYPE = r"(?:const\s+)?\w+(?:\s*\*(?:\s*const\b)?)*"
_SPACE = re.compile(r"\s*")
_STATEMENT = re.compile(r"[^;{}]*(?:\{[^{}]*\}[^;{}]*)?;")      # one declaration, with at most one brace pair
_DECL = re.compile(rf"({_TYPE})\s*\b(\w+(?:\s*,\s*\w+)*)")      # a type and the names declared with it


class HeaderError(ValueError):
    """The header holds something the reader does not fully understand."""


class Header(NamedTuple):
    constants: dict      # "ZETT_E_INVALID" -> -1: enumerators and integer #defines
    structs: dict        # "zett_dest" -> [("in", "void*"), ...], in header order
    functions: dict      # "zett_create" -> ("int", ["const zett_config*", "int", ...]), in header order


def parse(text: str, name: str = "<header>") -> Header:
    """Parse declarations; a text with an ``extern "C" {`` guard is read between the guard's two halves only."""
    blank = lambda s: " " + "\n" * s.count("\n")      # noqa: E731  (line numbers stay those of the file)
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: blank(m.group()), text, flags=re.S)      # comments hold ';', '(' and 'int'
    guard = re.search(r'#\s*ifdef\s+__cplusplus\s*\n\s*extern\s+"C"\s*\{\s*\n\s*#\s*endif[^\n]*\n', text)
    if guard:
        close = list(re.finditer(r"#\s*ifdef\s+__cplusplus\s*\n\s*\}\s*\n\s*#\s*endif", text))
        if not close or close[-1].start() < guard.end():
            raise HeaderError(f'{name}:{text.count(chr(10), 0, guard.start()) + 1}: extern "C" is never closed')
        text = blank(text[:guard.end()]) + text[guard.end():close[-1].start()] + blank(text[close[-1].start():])
    h = Header({}, {}, {})
    handles, spellings = [], {}      # handles: the opaque struct types; spellings: a type as written -> as returned, once it has been checked

    def fail(pos, why):
        line = text.count("\n", 0, pos) + 1
        raise HeaderError(f"{name}:{line}: {why}: {text.splitlines()[line - 1].strip()!r}")

    def constant(pos, key, value):
        if key in h.constants:
            fail(pos, f"{key} is defined twice")
        h.constants[key] = int(value)

    def ctype(pos, spelled):
        if spelled in spellings:
            return spellings[spelled]
        words = re.findall(r"\w+|\*", spelled)
        base = [w for w in words if w not in ("const", "*")]
        stars = words.count("*")
        known = SCALARS if not stars else POINTEES + tuple(handles) + tuple(h.structs)
        if len(base) != 1 or base[0] not in known or (not stars and "const" in words) or (base[0] == "char" and words != ["const", "char", "*"]):
            fail(pos, f"type {' '.join(spelled.split())!r} is outside the type table")
        spellings[spelled] = re.sub(r"\s*\*\s*", "* ", " ".join(words)).strip().replace("* *", "**")
        return spellings[spelled]

    def pieces(pos, body, sep):
        """(position, stripped text) of the sep-separated parts of body, which starts at pos"""
        for part in re.finditer(rf"[^{sep}]+|(?<={sep})(?={sep})", body):
            lead = len(part.group()) - len(part.group().lstrip())
            yield pos + part.start() + lead, part.group().strip()

    pos = 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos >= len(text):
            break
        if text[pos] == "#":
            end = text.find("\n", pos)
            end = len(text) if end < 0 else end
            m = re.fullmatch(rf"#\s*define\s+(\w+)\s+({_INT})\s*", text[pos:end])
            if not m:
                fail(pos, "not `#define NAME <decimal integer>`")
            constant(pos, m.group(1), m.group(2))
            pos = end
            continue
        m = _STATEMENT.match(text, pos)
        if not m:
            fail(pos, "not a declaration that ends in ';'")
        stmt, start, pos = m.group()[:-1], pos, m.end()
        if e := re.fullmatch(r"enum\s+\w+\s*\{([^{}]*)\}\s*", stmt):
            for at, item in pieces(start + e.start(1), e.group(1), ","):
                v = re.fullmatch(rf"(\w+)\s*=\s*({_INT})", item)
                if not v:
                    fail(at, "an enumerator needs an explicit decimal integer value")
                constant(at, v.group(1), v.group(2))
        elif e := re.fullmatch(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*", stmt):
            if e.group(1) != e.group(2) or e.group(1) in handles:
                fail(start, "an opaque handle is `typedef struct zett_x zett_x;`, once")
            handles.append(e.group(1))
        elif e := re.fullmatch(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*", stmt):
            if e.group(1) != e.group(3) or e.group(1) in h.structs:
                fail(start, "a struct is `typedef struct zett_x { ... } zett_x;`, once")
            fields = []
            for at, item in pieces(start + e.start(2), e.group(2), ";"):
                if not item:
                    continue      # what follows the last ';'
                d = _DECL.fullmatch(item)
                if not d:
                    fail(at, "a member is `type name[, name ...];` of scalar or pointer type")
                fields += [(n.strip(), ctype(at, d.group(1))) for n in d.group(2).split(",")]
            if not fields or len({n for n, _ in fields}) != len(fields):
                fail(start, "a struct needs members with distinct names")
            h.structs[e.group(1)] = fields
        elif e := re.fullmatch(rf"({_TYPE})\s*\b(\w+)\s*\(([^()]*)\)\s*", stmt):
            if e.group(2) in h.functions:
                fail(start, f"{e.group(2)} is declared twice")
            params = []
            if e.group(3).strip() != "void":
                for at, item in pieces(start + e.start(3), e.group(3), ","):
                    d = _DECL.fullmatch(item)
                    if not d or "," in d.group(2):
                        fail(at, "a parameter is `type name`")
                    params.append(ctype(at, d.group(1)))
            h.functions[e.group(2)] = (ctype(start, e.group(1)), params)
        else:
            fail(start, "neither an enum, a struct, an opaque handle nor a function declaration")
    return h


_header = None


def read() -> Header:
    """include/zett_hip.h, parsed once per process."""
    global _header
    if _header is None:
        with open(PATH) as f:
            _header = parse(f.read(), PATH)
    return _header
