"""The one place the tests compile against include/: what fovpt.h, compiled as C99 by gcc, says about its structs and constants
(the one copy of the program the *_cpu tests ask for sizeof / offsetof values and #define'd numbers), and the syntax check of a
piece of C or C++ that uses the headers."""
import os
import subprocess
import tempfile

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def _syntax_command(lang, include=()):
    return ["g++" if "+" in lang else "gcc", "-std=" + lang, "-fsyntax-only", "-I", INCLUDE] + [a for d in include for a in ("-I", d)]


def syntax_check(src, lang="c++14"):
    """The compiler's -fsyntax-only pass over the source text src as `lang` ("c++14", "c99": the -std value, which also picks g++
    or gcc) against include/; raises CalledProcessError with the compiler's messages on its standard error."""
    subprocess.run(_syntax_command(lang) + ["-x", "c++" if "+" in lang else "c", "-"], input=src.encode(), check=True)


def syntax_check_file(path, lang="c++14", include=()):
    """The same pass over a source file, against include/ and the directories of `include`."""
    subprocess.run(_syntax_command(lang, include) + [path], check=True)


def _members(mirror, rename):
    names = [f[0] for f in mirror._fields_] if hasattr(mirror, "_fields_") else list(mirror)
    return [rename.get(n, n) for n in names]


def probe(structs=(), constants=()):
    """structs: (C type name, mirror[, {mirror field: C member}]) each, the mirror a ctypes.Structure class or a sequence of member
    names; constants: C expressions of the header.  One program, compiled against include/fovpt.h and run.
    -> ([[sizeof, offsetof(member) ...] per struct, members in the mirror's order], [the constants' values as Python floats,
    exact for every integer below 2 ** 53 and every binary32 / binary64 number])."""
    body = []
    for cname, mirror, *rename in structs:
        body.append('printf("%%zu", sizeof(%s));' % cname)
        body += ['printf(" %%zu", offsetof(%s, %s));' % (cname, m) for m in _members(mirror, rename[0] if rename else {})]
        body.append('printf("\\n");')
    body += ['printf("%%a\\n", (double)(%s));' % c for c in constants]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "fovpt.h"\nint main(void){\n' + "\n".join(body) + "\nreturn 0;}\n"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "layout")
        subprocess.run(["gcc", "-std=c99", "-x", "c", "-I", INCLUDE, "-", "-o", exe], input=src.encode(), check=True)
        lines = subprocess.check_output([exe]).decode().splitlines()
    assert len(lines) == len(structs) + len(constants)
    return [[int(x) for x in line.split()] for line in lines[:len(structs)]], [float.fromhex(x) for x in lines[len(structs):]]


def layouts(*structs):
    """[sizeof, offsetof(member) ...] of each (C type name, mirror[, renames])."""
    return probe(structs)[0]


def layout(cname, mirror, rename=()):
    """[sizeof, offsetof(member) ...] of one struct."""
    return probe([(cname, mirror, dict(rename))])[0][0]


def offsets(mirror):
    """[sizeof, offset of every field ...] as the ctypes mirror has them: what layout() of its C type must equal."""
    import ctypes
    return [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]


def constants(*exprs):
    """The values of C constant expressions of the header."""
    return probe((), exprs)[1]
