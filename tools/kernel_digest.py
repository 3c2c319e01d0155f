"""Digest of the device code of a build: one line per gfx950 function symbol of every object under zett_amd/csrc/build/.

    python tools/kernel_digest.py [BUILD_DIR] > table.tsv

For each object: the .hip_fatbin section (llvm-objcopy --dump-section), its hipv4-amdgcn-amd-amdhsa--gfx950 code object
(clang-offload-bundler --unbundle), every FUNC symbol's (value, size) (llvm-readelf -s), and the sha256 of the symbol's bytes in
.text.  Columns: translation unit, symbol, size, sha256.  Two builds whose tables are equal run the same kernels; a host-only
change must leave the table as it was (profiles/forward_host_refactor.md).  Bytes are hashed, nothing is disassembled.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    tool("llvm-objcopy", "--dump-section", f".hip_fatbin={fatbin}", obj, os.path.join(tmp, "copy.o"))
    tool("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fatbin}", f"--output={co}")
    return co


def digests(obj):
    """[(symbol, size, sha256)] of the FUNC symbols of an object's gfx950 code object, by name."""
    if ".hip_fatbin" not in tool("llvm-readelf", "-S", "-W", obj):          # a unit of host code only (gemm_launch.hip)
        return []
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        text = re.search(r"^\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", tool("llvm-readelf", "-S", "-W", co), re.M)
        addr, offset = int(text.group(1), 16), int(text.group(2), 16)
        with open(co, "rb") as f:
            image = f.read()
        rows = set()          # (.dynsym and .symtab list every function: once here)
        for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$", tool("llvm-readelf", "-s", "-W", co), re.M):
            value, size, name = int(m.group(1), 16), int(m.group(2)), m.group(3)
            start = value - addr + offset
            rows.add((name, size, hashlib.sha256(image[start:start + size]).hexdigest()))
        return sorted(rows)


def main(build_dir):
    for obj in sorted(f for f in os.listdir(build_dir) if f.endswith(".o")):
        for name, size, sha in digests(os.path.join(build_dir, obj)):
            print(f"{obj[:-2]}\t{name}\t{size}\t{sha}")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "zett_amd", "csrc", "build"))
