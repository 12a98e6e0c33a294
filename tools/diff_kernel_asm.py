#!/usr/bin/env python3
"""Compare the device code of two builds of one .hip file, kernel by kernel.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S csrc/loss.hip -o new.s      (the same for the other tree -> old.s)
    python tools/diff_kernel_asm.py old.s new.s

Both files must define the same .amdhsa_kernel symbols, and every kernel's text from its label to its .Lfunc_end (instructions and
the kernel descriptor) must be equal once comments, the compilation-unit id and the ordinals of local labels are taken out.
Exit status 0 when they are; prints the symbol count."""
import re
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M):
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), txt, re.M | re.S)
        body = re.sub(r"[ \t]*;[^\n]*|[ \t]+$", "", m.group(1), flags=re.M)      # comments and the padding in front of them
        body = re.sub(r"__hip_cuid_\w+", "CUID", body)
        out[sym] = re.sub(r"\.L([A-Za-z_]*)\d+(_\d+)?", r".L\1", body)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only = sorted(set(a) ^ set(b))
    differ = sorted(s for s in a if s in b and a[s] != b[s])
    print(f"{len(a)} / {len(b)} kernel symbols, {sum(v.count(chr(10)) for v in a.values())} lines compared; "
          f"in one file only: {only}; differing: {differ}")
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main())
