"""Writes tests/golden/detmath_vectors.npz and tests/golden/detmath_frozen.json (run by hand; needs mpmath, g++ and git).

    python tests/golden/make_detmath_golden.py vectors            # mpmath at 200 bits -> detmath_vectors.npz
    python tests/golden/make_detmath_golden.py frozen REV         # include/fovpt_detmath.h as of git revision REV -> detmath_frozen.json

vectors: for every op, the slice detmath_cases.golden_subset() of the structured inputs with the correctly rounded binary32
result (`cr`) and the value itself as a float64 pair hi + lo.  Results that are zeros, infinities or NaN come from the
rule tables below (C99 Annex F and the header's documented branches), not from mpmath, which has no signed zero.

frozen: a sha256 per op over the output bits on the `frozen` inputs, computed with the header of an EARLIER revision compiled by
g++ -O2 -ffp-contract=off -- never with the working tree's header, which is the code under test.  The file names the revision.
"""
import ctypes
import hashlib
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import detmath_cases as dc  # noqa: E402
from fovpathtracing_optixcodelatest_amd import abi  # noqa: E402

f32 = np.float32
NAN, INF = float("nan"), float("inf")


def special(op, a, b):
    """The result where it is a zero, an infinity or NaN by rule; None where it is an ordinary number to compute."""
    neg = lambda v: math.copysign(1.0, v) < 0
    if op in (abi.OP_SIN, abi.OP_SQRT) and a == 0:
        return a                                                # +-0 -> +-0
    if op == abi.OP_ACOS and a == 1:
        return 0.0
    if op == abi.OP_ATAN2 and a == 0 and not neg(b):            # C99 F.9.1.4: atan2(+-0, +0 or x > 0) = +-0
        return math.copysign(0.0, a)
    if op == abi.OP_LOG:
        if math.isnan(a) or a < 0:
            return NAN
        if a == 0:
            return -INF
        if a == INF:
            return INF
        if a == 1:
            return 0.0
    if op == abi.OP_SQRT:
        if math.isnan(a) or a < 0:
            return NAN
        if a == INF:
            return INF
    if op == abi.OP_POW:                                        # the header's branches, in its order
        if math.isnan(a) or math.isnan(b):
            return NAN
        if b == 0:
            return 1.0
        if a == 0:
            return 0.0 if b > 0 else INF
        if a < 0:
            return NAN
        if a == 1:
            return 1.0
        if math.isinf(b):
            return INF if (a > 1) == (b > 0) else 0.0
    if op == abi.OP_DIV:
        if math.isnan(a) or math.isnan(b) or (a == 0 and b == 0) or (math.isinf(a) and math.isinf(b)):
            return NAN
        s = -1.0 if neg(a) != neg(b) else 1.0
        if math.isinf(a) or b == 0:
            return s * INF
        if math.isinf(b) or a == 0:
            return s * 0.0
    return None


def value(mp, op, a, b):
    x = mp.mpf(a)
    if op == abi.OP_SIN:
        return mp.sin(x)
    if op == abi.OP_COS:
        return mp.cos(x)
    if op == abi.OP_ACOS:
        return mp.acos(x)
    if op == abi.OP_ATAN2:
        if a == 0:                                              # atan2(+-0, -0 or x < 0) = +-pi
            return mp.pi if math.copysign(1.0, a) > 0 else -mp.pi
        if b == 0:                                              # atan2(y, +-0) = +-pi/2
            return mp.sign(x) * mp.pi / 2
        return mp.atan2(x, mp.mpf(b))
    if op == abi.OP_LOG:
        return mp.log(x)
    if op == abi.OP_POW:
        return mp.exp(mp.mpf(b) * mp.log(x))
    if op == abi.OP_SQRT:
        return mp.sqrt(x)
    if op == abi.OP_DIV:
        return x / mp.mpf(b)
    raise ValueError(op)


def round_to_binary32(mp, v):
    """Round-to-nearest-even of the mpf v (finite, non-zero) to binary32, subnormals and overflow included."""
    av = abs(v)
    _, e = mp.frexp(av)                                         # av = m * 2**e, m in [0.5, 1)
    q = max(int(e) - 1, -126) - 23
    n = int(mp.nint(mp.ldexp(av, -q)))                          # ties to even
    r = math.ldexp(n, q)                                        # exact: n <= 2**24
    if r >= 2.0 ** 128:
        r = INF
    return math.copysign(r, 1.0 if v > 0 else -1.0)


def make_vectors():
    import mpmath
    mp = mpmath.mp
    mp.prec = 200
    out = {}
    for op in dc.ALL_OPS:
        name = dc.NAMES[op]
        c = dc.cases(op)
        idx = dc.golden_subset(op)
        a = c.a[idx]
        b = c.b[idx] if c.b is not None else None
        cr = np.empty(idx.size, f32)
        hi = np.empty(idx.size, np.float64)
        lo = np.zeros(idx.size, np.float64)
        by_rule = 0
        for i in range(idx.size):
            ai, bi = float(a[i]), (float(b[i]) if b is not None else None)
            s = special(op, ai, bi)
            if s is not None:
                cr[i], hi[i] = s, s
                by_rule += 1
                continue
            v = value(mp, op, ai, bi)
            cr[i] = round_to_binary32(mp, v)
            h = float(v)
            hi[i] = h
            if math.isfinite(h):
                lo[i] = float(v - mp.mpf(h))
            if cr[i] == 0:                                      # underflow keeps the value's sign
                cr[i] = math.copysign(0.0, 1.0 if v > 0 else -1.0)
        out[name + "_a"] = a
        if b is not None:
            out[name + "_b"] = b
        out[name + "_cr"], out[name + "_hi"], out[name + "_lo"] = cr, hi, lo
        print("%-6s %5d points, %d by rule" % (name, idx.size, by_rule))
    path = os.path.join(HERE, "detmath_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


SHIM = r"""
#include <stddef.h>
#include "fovpt_detmath.h"
extern "C" void dm(int op, size_t n, const float* a, const float* b, float* out)
{
    for (size_t i = 0; i < n; i++) {
        switch (op) {
        case 1: out[i] = fovpt_dm_sinf(a[i]); break;
        case 2: out[i] = fovpt_dm_cosf(a[i]); break;
        case 3: out[i] = fovpt_dm_acosf(a[i]); break;
        case 4: out[i] = fovpt_dm_atan2f(a[i], b[i]); break;
        case 5: out[i] = fovpt_dm_logf(a[i]); break;
        case 6: out[i] = fovpt_dm_powf(a[i], b[i]); break;
        }
    }
}
"""


def make_frozen(rev):
    sha = subprocess.check_output(["git", "-C", ROOT, "rev-parse", rev + "^{commit}"], text=True).strip()
    header = subprocess.check_output(["git", "-C", ROOT, "show", sha + ":include/fovpt_detmath.h"])
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "fovpt_detmath.h"), "wb") as f:
            f.write(header)
        with open(os.path.join(tmp, "shim.cpp"), "w") as f:
            f.write(SHIM)
        so = os.path.join(tmp, "shim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-I", tmp,
                               "-o", so, os.path.join(tmp, "shim.cpp")])
        L = ctypes.CDLL(so)
        L.dm.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        digests = {}
        for op in dc.FROZEN_OPS:
            c = dc.cases(op)
            out = np.empty_like(c.a)
            L.dm(op, c.a.size, c.a.ctypes.data, c.b.ctypes.data if c.b is not None else None, out.ctypes.data)
            assert not np.isnan(out[c.frozen]).any()
            digests[dc.NAMES[op]] = {"inputs": int(c.frozen.sum()), "sha256": dc.frozen_digest(op, out)}
        # the stand-alone sweep's digest of every 64th float's sin and cos bits in [0, 2 pi], from the same old header
        exe = os.path.join(tmp, "detmath_sweep")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-I", tmp,
                               os.path.join(ROOT, "tests", "cpp", "detmath_sweep.cpp"), "-o", exe])
        text = subprocess.check_output([exe, "64"], text=True)
        sweep = [ln.split("=")[1] for ln in text.splitlines() if ln.startswith("sincos_digest=")][0]
    doc = {"header": "include/fovpt_detmath.h", "revision": sha, "header_sha256": hashlib.sha256(header).hexdigest(),
           "compiler": "g++ -O2 -ffp-contract=off", "ops": digests, "sweep_sincos_stride64": sweep}
    path = os.path.join(HERE, "detmath_frozen.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "vectors":
        make_vectors()
    elif len(sys.argv) == 3 and sys.argv[1] == "frozen":
        make_frozen(sys.argv[2])
    else:
        sys.exit(__doc__)
