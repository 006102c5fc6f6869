#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of one translation unit, function by function.

    tools/codeobj_diff.py PARENT/csrc/wavefront.o csrc/wavefront.o [name-substring ...]

Takes the code object out of each object file (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle),
reads every function symbol's bytes from .text and every kernel descriptor from .rodata, and prints which are identical.
The files as a whole always differ once the source does: hipcc puts a symbol named after a hash of the source
(__hip_cuid_...) into every code object.  Exit status 1 when a function or descriptor that was asked for (default: all)
differs or exists on one side only.  Needs no GPU."""
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def code_object(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fat"), os.path.join(tmp, tag + ".co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    bundler = os.path.join(LLVM, "clang-offload-bundler")
    targets = subprocess.check_output([bundler, "--list", "--type=o", "--input=" + fat], text=True).split()
    gpu = [t for t in targets if "gfx" in t]
    assert len(gpu) == 1, targets
    subprocess.check_call([bundler, "--unbundle", "--type=o", "--input=" + fat, "--targets=" + gpu[0], "--output=" + co])
    return co


def symbols(co):
    """name -> bytes, for the functions in .text and the kernel descriptors (*.kd) in .rodata"""
    readelf = os.path.join(LLVM, "llvm-readelf")
    sect = {}
    for line in subprocess.check_output([readelf, "-SW", co], text=True).splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[0].isdigit() and f[1] in (".text", ".rodata"):
            sect[int(f[0])] = (int(f[3], 16), int(f[4], 16))          # index -> (address, file offset)
    data = open(co, "rb").read()
    out = {}
    for line in subprocess.check_output([readelf, "-sW", co], text=True).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit() and int(f[6]) in sect:
            if f[3] == "OBJECT" and not f[7].endswith(".kd"):
                continue
            addr, off = sect[int(f[6])]
            start = int(f[1], 16) - addr + off
            out[f[7]] = data[start:start + int(f[2])]
    return out


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        a, b = symbols(code_object(argv[1], tmp, "a")), symbols(code_object(argv[2], tmp, "b"))
    wanted = argv[3:]
    bad = 0
    for name in sorted(set(a) | set(b)):
        if wanted and not any(w in name for w in wanted):
            continue
        if name not in a or name not in b:
            state = "only in " + (argv[1] if name in a else argv[2])
        elif a[name] == b[name]:
            state = "identical (%d bytes)" % len(a[name])
        else:
            state = "DIFFERENT (%d / %d bytes)" % (len(a[name]), len(b[name]))
        bad += not state.startswith("identical")
        print("%-110s %s" % (name, state))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
