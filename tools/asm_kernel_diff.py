#!/usr/bin/env python3
"""Compare two ISA listings of one translation unit (`make -C vulkan-compute-tests_amd asm`, build/asm/<file>.s) kernel by kernel:
each kernel's section runs from its label to its .Lfunc_end line (the code, the kernel descriptor, the resource comments).  Prints
which kernels of the first listing are identical, differ or are missing in the second, and the kernels only the second has; exits 1
unless every kernel of the first listing is identical in the second.

    python tools/asm_kernel_diff.py parent/build/asm/mandelbrot.s vulkan-compute-tests_amd/build/asm/mandelbrot.s
"""
import re
import sys


def sections(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        if name is not None:
            body.append(line)
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = sections(sys.argv[1]), sections(sys.argv[2])
    bad = 0
    for name, body in a.items():
        state = "missing" if name not in b else "identical" if b[name] == body else "DIFFERS"
        bad += state != "identical"
        print(f"{state:9s} {name}")
    for name in b:
        if name not in a:
            print(f"{'new':9s} {name}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
