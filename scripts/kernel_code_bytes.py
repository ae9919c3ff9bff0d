#!/usr/bin/env python3
"""Code bytes per kernel of two builds of liblmc_hip.so, side by side: the sizes of the kernels' function symbols in the gfx950 code objects the library
embeds (its .hip_fatbin section: one offload bundle per translation unit).  Complements scripts/kernel_resources_diff.py, whose remarks carry no code size.

    python scripts/kernel_code_bytes.py <parent liblmc_hip.so> <this tree's liblmc_hip.so> >> profiles/<name>.txt

Needs llvm-objcopy, clang-offload-bundler and llvm-readelf of the ROCm LLVM (ROCM_LLVM_BIN, default /opt/rocm/llvm/bin) and c++filt.  A kernel is a FUNC symbol
that has a `<name>.kd` descriptor object beside it.  Kernels of the same mangled name in two units (anonymous namespaces) are listed once per unit, in file order."""
import os
import re
import subprocess
import sys
import tempfile

BIN = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(lib):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([os.path.join(BIN, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for k, s in enumerate(starts):
            bundle, co = os.path.join(d, "b%d" % k), os.path.join(d, "co%d" % k)
            open(bundle, "wb").write(blob[s:starts[k + 1] if k + 1 < len(starts) else len(blob)])
            r = subprocess.run([os.path.join(BIN, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + co],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            sym = subprocess.run([os.path.join(BIN, "llvm-readelf"), "-s", "-W", co], stdout=subprocess.PIPE, text=True, check=True).stdout
            size, kd = {}, set()
            for line in sym.splitlines():
                f = line.split()
                if len(f) < 8 or not f[0].endswith(":") or not f[2].isdigit():
                    continue
                if f[3] == "FUNC":
                    size[f[7]] = int(f[2])
                elif f[7].endswith(".kd"):
                    kd.add(f[7][:-3])
            for n in sorted(kd):
                if n in size:
                    out.setdefault(n, []).append(size[n])
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(set(a) | set(b))
    dem = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    rows = sorted(zip((re.sub(r"^void ", "", re.sub(r"\((?!anonymous namespace\)).*", "", d)) for d in dem), names))
    differ = only_b = 0
    print("\n## Code bytes per kernel (function symbol sizes in the embedded gfx950 code objects): first library -> second library")
    for d, n in rows:
        x, y = a.get(n), b.get(n)
        if x is None:
            only_b += 1
            print("    %-140s | only in the second: %s" % (d, ", ".join(map(str, y))))
        elif y is None:
            print("    %-140s | only in the first: %s" % (d, ", ".join(map(str, x))))
        else:
            mark = "" if x == y else "   <-- differs"
            differ += x != y
            print("    %-140s | %s -> %s%s" % (d, ", ".join(map(str, x)), ", ".join(map(str, y)), mark))
    print("\nkernels in both libraries: %d, of them with different code bytes: %d; only in the second: %d" % (len(set(a) & set(b)), differ, only_b))


if __name__ == "__main__":
    main()
