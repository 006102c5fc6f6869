"""The cases fovpt_quality_host is compared with tests/quality_ref.py on (tests/test_quality_cpu.py, and the sanitizer program
tests/cpp/quality_host_test.cpp): edge sizes, gazes in and off the frame, ring widths, every flag combination, image pairs with a
known answer, class maps with all five classes and with one absent."""
import ctypes as C
import itertools
import struct

import numpy as np

import quality_ref as qr
from fovpathtracing_optixcodelatest_amd import abi

SIZES = [(1, 1), (7, 9), (8, 8), (11, 12), (12, 8), (37, 61), (70, 45)]
IMAGES = ["random", "identical", "black_white", "checker", "alpha"]
CLASS_MAPS = ["all_five", "one_absent"]
RING_WIDTHS = [1, 16, 65536]
FLAGS = [0, qr.SSIM, qr.PROFILE, qr.SSIM | qr.PROFILE]
GAZES = ["centre", "origin", "off_positive", "off_negative", "int32_min"]


def gaze_of(kind, w, h):
    """The gaze as the uint32 pair a launch holds; the last two are negative as int32."""
    u32 = lambda v: v & 0xffffffff
    return {"centre": (w // 2, h // 2), "origin": (0, 0), "off_positive": (w + 40, h + 13), "off_negative": (u32(-9), u32(-3)),
            "int32_min": (0x80000000, 5)}[kind]


def images_of(kind, w, h, rng):
    rand = lambda: rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    if kind == "random":
        return rand(), rand()
    if kind == "identical":
        a = rand()
        return a, a.copy()
    if kind == "black_white":
        return rand() & np.uint32(0xff000000), rand() | np.uint32(0x00ffffff)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.where((xx + yy) % 2 == 0, 0x00ffffff, 0).astype(np.uint32)
        return a | np.uint32(0xff000000), (a ^ np.uint32(0x00ffffff))
    if kind == "alpha":
        a = rand()
        return a, a ^ (rand() & np.uint32(0xff000000))
    raise ValueError(kind)


def classes_of(kind, w, h, rng):
    pool = np.arange(5, dtype=np.uint8) if kind == "all_five" else np.array([0, 1, 2, 4], np.uint8)      # (one_absent: no UNIFORM)
    k = rng.choice(pool, (h, w))
    if w * h >= len(pool):
        k.reshape(-1)[rng.permutation(w * h)[:len(pool)]] = pool
    return k.astype(np.uint8)


def cases():
    """-> dicts with label, w, h, gaze (uint32 pair), cfg, test, ref, classes.  Every (size, image, class map) with four of the
    (gaze, ring width, flags) combinations, taken in turn: every combination comes up."""
    combos = list(itertools.product(GAZES, RING_WIDTHS, FLAGS))
    out = []
    for i, ((w, h), image, cmap) in enumerate(itertools.product(SIZES, IMAGES, CLASS_MAPS)):
        rng = np.random.default_rng(500 + i)
        test, ref = images_of(image, w, h, rng)
        classes = classes_of(cmap, w, h, rng)
        for j in range(4):
            gaze, rw, flags = combos[(4 * i + j) % len(combos)]
            out.append(dict(label="%dx%d %s %s %s rw%d f%d" % (w, h, image, cmap, gaze, rw, flags), w=w, h=h, image=image, class_map=cmap,
                            gaze=gaze_of(gaze, w, h), cfg=dict(flags=flags, ring_width=rw), test=test, ref=ref, classes=classes))
    assert len(out) >= len(combos)
    return out


def sums_of_dict(d):
    """The abi.QualitySums holding the fields of a quality_ref.quality() result."""
    s = abi.QualitySums()
    for name, _ in abi.QualitySums._fields_:
        v = d[name]
        if name == "sq_err":
            for k in range(5):
                for c in range(3):
                    s.sq_err[k][c] = v[k][c]
        elif isinstance(v, list):
            for k, x in enumerate(v):
                getattr(s, name)[k] = x
        else:
            setattr(s, name, v)
    return s


def config_of(cfg):
    c = abi.QualityConfig()
    c.flags, c.ring_width = int(cfg["flags"]), int(cfg["ring_width"])
    return c


def host_quality(L, test, ref, classes, gaze, cfg):
    """fovpt_quality_host of library L -> (return code, abi.QualitySums)."""
    test, ref = np.ascontiguousarray(test, np.uint32), np.ascontiguousarray(ref, np.uint32)
    h, w = test.shape
    k = np.ascontiguousarray(classes, np.uint8) if classes is not None else None
    s = abi.QualitySums()
    rc = L.fovpt_quality_host(test.ctypes.data, ref.ctypes.data, w, h, k.ctypes.data if k is not None else None, qr.as_int32(gaze[0]),
                              qr.as_int32(gaze[1]), C.byref(config_of(cfg)), C.byref(s))
    return rc, s


def write_cases(path, cs):
    """The file tests/cpp/quality_host_test.cpp reads: per case int32 w, h, flags, ring_width, int64 gaze x, y, the two images, the
    classes, and the 1344 bytes of the record quality_ref gives."""
    with open(path, "wb") as f:
        for c in cs:
            want = sums_of_dict(qr.quality(c["test"], c["ref"], c["classes"], c["gaze"], c["cfg"]))
            f.write(struct.pack("<iiiiqq", c["w"], c["h"], c["cfg"]["flags"], c["cfg"]["ring_width"], qr.as_int32(c["gaze"][0]), qr.as_int32(c["gaze"][1])))
            f.write(c["test"].tobytes() + c["ref"].tobytes() + c["classes"].tobytes() + bytes(want))
