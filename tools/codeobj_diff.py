#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds, object file by object file.

    tools/codeobj_diff.py OLD/_lib/obj NEW/_lib/obj

For every *.o present in both directories that carries device code, the gfx950
code object is pulled out of .hip_fatbin and four things are compared: the
bytes of .text, the bytes of .rodata (kernel descriptors), the sorted list of
(function symbol, size), and the kernel metadata notes (register, spill, LDS
and scratch figures).  One line per file: `identical`, or which of the four
differ.  Instruction bytes are only ever compared, never decoded.  Exit status
1 on any difference.  CPU only; needs the ROCm LLVM tools.
"""
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def section(elf, name, tmp):
    out = os.path.join(tmp, "sec.bin")
    run("llvm-objcopy", "-O", "binary", f"--only-section={name}", elf, out)
    with open(out, "rb") as f:
        return f.read()


def parts(obj, tmp):
    """(.text, .rodata, function symbols, notes) of obj's gfx950 code object, or None without device code."""
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co.elf")
    run("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    run("clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}", f"--targets={TARGET}", f"--output={co}")
    syms = sorted((f[7], int(f[2])) for f in (l.split() for l in run("llvm-readelf", "--symbols", "--wide", co).splitlines())
                  if len(f) == 8 and f[3] == "FUNC")
    if not syms:
        return None
    return section(co, ".text", tmp), section(co, ".rodata", tmp), syms, run("llvm-readelf", "--notes", co)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = sys.argv[1:]
    names = sorted(n for n in os.listdir(old) if n.endswith(".o"))
    only = sorted(set(n for n in os.listdir(new) if n.endswith(".o")) ^ set(names))
    bad = len(only)
    for n in only:
        print(f"{n:24s} in one directory only")
    for n in names:
        if n in only:
            continue
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            a, b = parts(os.path.join(old, n), ta), parts(os.path.join(new, n), tb)
        if a is None and b is None:
            continue  # host code only
        if a is None or b is None:
            diff = ["device code in one build only"]
        else:
            diff = [w for w, x, y in zip((".text", ".rodata", "symbols", "metadata"), a, b) if x != y]
        bad += bool(diff)
        size = f"{len(b[0]):>9d} B .text" if b else ""
        print(f"{n:24s} {size}  " + ("identical" if not diff else "DIFFERENT: " + ", ".join(diff)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
