"""Writes tests/golden/forward_launch_log.json: what the forward's host orchestration did, per case of tests/forward_launch_cases.py,
on a library built from the commit BEFORE the change under test.

    ZETT_HIP_LIB=/path/to/parent/libzett_hip.so python tests/golden/make_golden_forward_launch_log.py [--out FILE]

Run once, on an MI355X.  ZETT_HIP_LIB selects the library (zett_amd/_lib.py); a file SOURCE_HASH beside it holds
`zett_amd.build.source_hash()` of the tree it was built from.  The generator refuses a library built from the working tree: no
ZETT_HIP_LIB, the tree's own libzett_hip.so, or a SOURCE_HASH equal to the working tree's.  It is never run against the code under test.
Every case runs twice; an output digest that does not repeat is dropped (null) and the case listed under "unreproducible".
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))


def parent_hash():
    from zett_amd import build
    lib = os.environ.get("ZETT_HIP_LIB")
    if not lib:
        sys.exit("ZETT_HIP_LIB is not set: the fixture is recorded on a library built from the parent commit")
    if os.path.realpath(lib) == os.path.realpath(build.LIB_PATH):
        sys.exit(f"{lib} is the working tree's own library")
    stamp = os.path.join(os.path.dirname(os.path.abspath(lib)), "SOURCE_HASH")
    if not os.path.exists(stamp):
        sys.exit(f"{stamp} is missing: write zett_amd.build.source_hash() of the parent tree there")
    with open(stamp) as f:
        recorded = f.read().strip()
    if recorded == build.source_hash():
        sys.exit(f"{lib} was built from the sources of the working tree ({recorded}): nothing to compare against")
    return recorded


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "forward_launch_log.json"))
    args = ap.parse_args()
    recorded = parent_hash()
    from tests import forward_launch_cases as cases
    out = {"parent_source_hash": recorded, "unreproducible": [], "cases": {}}
    for name in cases.CASES:
        first, second = cases.run_case(name), cases.run_case(name)
        for key in ("gemm_log", "stats", "workspace_bytes"):
            assert first[key] == second[key], (name, key)
        if first["outputs"] != second["outputs"]:
            out["unreproducible"].append(name)
            first["outputs"] = [a if a == b else None for a, b in zip(first["outputs"], second["outputs"])]
        out["cases"][name] = first
        print(name, len(first["gemm_log"]), "launches", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", args.out, "unreproducible:", out["unreproducible"])


if __name__ == "__main__":
    main()
