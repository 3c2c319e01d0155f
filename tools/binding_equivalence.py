"""Is the binding zett_amd/_lib.py derives from include/zett_hip.h the one another revision wrote out by hand?

    python tools/binding_equivalence.py [REV]          (default HEAD~1; no GPU and no built library needed)

Loads REV's zett_amd/_lib.py and this tree's side by side, each over a stand-in for ctypes.CDLL that only records the prototypes load()
declares, and compares: constants (REV's are a subset, same values), ABI_SYMBOLS, the ctypes.Structure classes (names, fields, types,
offsets, sizes) and every function's restype and argtypes position by position.  The one difference it lets pass, and lists: a
POINTER(scalar) parameter that is c_void_p now.  Exit status 1 on any other.  profiles/binding_refactor.md holds a run.
"""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


class _Function:
    restype, argtypes = C.c_int, None      # what ctypes gives a function nobody declared

    def __call__(self, *args):
        return self.version


class _Library:
    def __init__(self, path):
        pass

    def __getattr__(self, name):
        if not name.startswith("zett_"):
            raise AttributeError(name)
        self.__dict__[name] = _Function()
        return self.__dict__[name]


def loaded(module):
    """module.load() over the stand-in library: (module, {function name: (restype, argtypes)})"""
    _Function.version = module.ABI_VERSION
    real, C.CDLL, module.lib_path = C.CDLL, _Library, lambda: __file__
    try:
        lib = module.load()
    finally:
        C.CDLL = real
    return {n: (f.restype, list(f.argtypes or ())) for n, f in vars(lib).items()}


def module_at(rev):
    text = subprocess.run(["git", "show", f"{rev}:zett_amd/_lib.py"], cwd=REPO, check=True, capture_output=True, text=True).stdout
    spec = importlib.util.spec_from_loader("zett_amd._lib_at_rev", loader=None)
    module = importlib.util.module_from_spec(spec)
    module.__package__ = "zett_amd"
    exec(compile(text, f"{rev}:zett_amd/_lib.py", "exec"), module.__dict__)
    return module


def structures(module):
    return {n: c for n, c in vars(module).items() if isinstance(c, type) and issubclass(c, C.Structure)}


def main(rev):
    import zett_amd      # noqa: F401  (the package REV's module is a member of)
    from zett_amd import _lib as new
    old = module_at(rev)
    bad = []

    ints = lambda m: {n: v for n, v in vars(m).items() if type(v) is int and n.isupper()}      # noqa: E731
    old_c, new_c = ints(old), ints(new)
    bad += [f"constant {n}: {v} -> {new_c.get(n)}" for n, v in old_c.items() if new_c.get(n) != v]
    print(f"constants: {len(old_c)} of {rev} all present with the same value: {not bad}; {len(new_c)} now, new: {sorted(set(new_c) - set(old_c))}")

    same = sorted(old.ABI_SYMBOLS) == sorted(new.ABI_SYMBOLS)
    print(f"ABI_SYMBOLS: {len(old.ABI_SYMBOLS)} -> {len(new.ABI_SYMBOLS)}, same names: {same}, same order: {tuple(old.ABI_SYMBOLS) == tuple(new.ABI_SYMBOLS)}")
    if not same:
        bad.append(f"ABI_SYMBOLS differ: {sorted(set(old.ABI_SYMBOLS) ^ set(new.ABI_SYMBOLS))}")

    old_s, new_s = structures(old), structures(new)
    if sorted(old_s) != sorted(new_s):
        bad.append(f"structures differ: {sorted(set(old_s) ^ set(new_s))}")
    for n in sorted(set(old_s) & set(new_s)):
        layout = lambda c: [(f, t, getattr(c, f).offset, getattr(c, f).size) for f, t in c._fields_]      # noqa: E731
        ok = layout(old_s[n]) == layout(new_s[n]) and C.sizeof(old_s[n]) == C.sizeof(new_s[n])
        print(f"struct {n}: {len(new_s[n]._fields_)} fields, {C.sizeof(new_s[n])} bytes, same names, types, offsets and size: {ok}")
        if not ok:
            bad.append(f"struct {n}: {layout(old_s[n])} -> {layout(new_s[n])}")

    old_f, new_f = loaded(old), loaded(new)
    loosened = []
    for n in new.ABI_SYMBOLS:
        (r0, a0), (r1, a1) = old_f[n], new_f[n]
        if r0 is not r1 or len(a0) != len(a1):
            bad.append(f"{n}: restype {r0} -> {r1}, {len(a0)} -> {len(a1)} parameters")
            continue
        for i, (t0, t1) in enumerate(zip(a0, a1)):
            if t0 is t1:
                continue
            if t1 is C.c_void_p and issubclass(t0, C._Pointer) and not issubclass(t0._type_, C.Structure):
                loosened.append(f"{n}[{i}] POINTER({t0._type_.__name__})")
            elif issubclass(t0, C._Pointer) and issubclass(t1, C._Pointer) and t0._type_.__name__ == t1._type_.__name__ and old_s[t0._type_.__name__] is t0._type_:
                continue      # POINTER(ZettDest) of either module: the structures were compared above
            else:
                bad.append(f"{n}[{i}]: {t0} -> {t1}")
    declared = sum(1 for r, a in old_f.values() if a)
    print(f"functions: {len(new_f)} ({declared} with parameters declared in {rev}), restype and argtypes equal position by position: {not bad}")
    print(f"POINTER(scalar) -> c_void_p, {len(loosened)} positions:")
    for line in loosened:
        print("  " + line)
    for line in bad:
        print("MISMATCH " + line)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "HEAD~1"))
