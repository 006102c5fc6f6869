"""What the depth packet's and fovpt_warp_depth's tests on the CPU and on the GPU share: the camera, the synthetic G-buffers and
depth images, and the one-field mutations of a depth packet.  The shapes are packet_cases.SHAPES."""
import struct

import numpy as np

import packet_depth_ref as pd
import temporal_ref as tr
from fovpathtracing_optixcodelatest_amd import renderer

from gpu_common import BOX_CAMERA

MISS = np.uint32(0xffffffff)
JUNK_DEPTH = np.float32(-7.25)                   # (a value no decoder writes: depths are positive or +inf)


def camera_dict(size, eye=None, lookat=None, base=BOX_CAMERA):
    """The dict of eye / U / V / W the restatements take, of the box scene's camera (or another eye / lookat) at this size."""
    cam = renderer.Camera(eye or base["eye"], lookat or base["lookat"], base["up"], base["fovy"], size[0] / float(size[1]))
    to = renderer.SampleRenderer.warp_camera(cam)
    vec = lambda v: (float(v.x), float(v.y), float(v.z))
    return dict(eye=vec(to.eye), U=vec(to.U), V=vec(to.V), W=vec(to.W))


def synthetic_gbuffer(size, cam, seed, sky_blocks=True):
    """A G-buffer no scene gives: points on the pixels' own rays at depths log-uniform over [0.01, 1e5], and among them points
    behind the camera, NaN and infinite positions and sky -- single sky pixels, and 8 x 8 blocks of sky whose borders cut
    through texels.  -> dict prim (h, w) uint32, position (h, w, 4) float32."""
    w, h = size
    rng = np.random.default_rng(seed)
    z = np.exp(rng.uniform(np.log(0.01), np.log(1e5), (h, w)))
    kind = rng.integers(0, 100, (h, w))
    z = np.where(kind < 4, -z, z)                                         # behind the camera
    r = tr.miss_dirs(w, h, cam["U"], cam["V"], cam["W"]).astype(np.float64)
    X = (np.asarray(cam["eye"], np.float64) + z[..., None] * r).astype(np.float32)
    X[kind == 4] = np.nan
    X[kind == 5, 0] = np.inf
    X[kind == 6] = -np.inf
    X[kind == 7] = np.asarray(cam["eye"], np.float32)                     # z = 0
    prim = rng.integers(0, 1000, (h, w)).astype(np.uint32)
    prim[(kind >= 8) & (kind < 14)] = MISS
    if sky_blocks:
        for _ in range(6):
            x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8))
            prim[y0:y0 + 8, x0:x0 + 8] = MISS
            x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8))
            prim[y0:y0 + 8, x0:x0 + 8] = 7                                # and blocks that are all hits
            X[y0:y0 + 8, x0:x0 + 8] = (np.asarray(cam["eye"], np.float64) + 3.0 * r[y0:y0 + 8, x0:x0 + 8]).astype(np.float32)
    pos = np.concatenate([X, np.ones((h, w, 1), np.float32)], axis=-1)
    return dict(prim=prim, position=np.ascontiguousarray(pos, np.float32))


def synthetic_depth(size, seed):
    """A depth image with everything fovpt_warp_depth must tell apart: depths log-uniform over [0.01, 1e5], +inf, NaN, 0, -0,
    negatives and -inf."""
    w, h = size
    rng = np.random.default_rng(seed)
    z = np.exp(rng.uniform(np.log(0.01), np.log(1e5), (h, w))).astype(np.float32)
    kind = rng.integers(0, 100, (h, w))
    for k, v in enumerate((np.inf, np.nan, 0.0, -0.0, -1.5, -np.inf)):
        z[kind == k] = v
    z[kind == 6] = np.inf
    z[(kind >= 7) & (kind < 40)] = np.float32(4.0)                        # a plane, so that neighbours land side by side
    return z


def junk_depth(size):
    return np.full((size[1], size[0]), JUNK_DEPTH, np.float32)


def mutations(packet):
    """(label, mutated packet) for every rejection fovpt_packet_check_depth lists: one field of a valid packet changed each."""
    w = list(struct.unpack("<48I", packet[:192]))
    npass = w[6]
    body = packet[192:]

    def put(i, v):
        m = list(w)
        m[i] = v & 0xffffffff
        return struct.pack("<48I", *m) + body

    bits = lambda f: struct.unpack("<I", struct.pack("<f", f))[0]
    out = [("magic", put(0, w[0] ^ 1)), ("the colour magic", put(0, 0x4b505646)), ("the coded magic", put(0, 0x43505646)),
           ("version 0", put(1, 0)), ("version 2", put(1, 2)),
           ("bytes above the bytes given", put(2, w[2] + 4)), ("bytes below 192", put(2, 188)), ("bytes 128", put(2, 128)), ("bytes 0", put(2, 0)),
           ("width 0", put(4, 0)), ("width -1", put(4, -1)), ("width 16385", put(4, 16385)), ("another width", put(4, w[4] + 1)),
           ("height 0", put(5, 0)), ("height 16385", put(5, 16385)), ("another height", put(5, w[5] - 1)),
           ("npass 0", put(6, 0)), ("npass 4", put(6, 4)), ("reserved", put(7, 1))]
    if npass < 3:
        out += [("npass + 1 over a zero entry", put(6, npass + 1))]
        out += [("unused pass entry word %d" % k, put(8 + 8 * npass + k, 1)) for k in range(8)]
    p = 8 + 8 * (npass - 1)                       # the last pass
    out += [("eighth pass word 1", put(p + 7, 1)), ("eighth pass word of the first pass", put(15, 1)), ("gw 0", put(p + 0, 0)), ("gh 0", put(p + 1, 0)),
            ("too many texels", put(p + 1, (1 << 26) // w[p + 0] + 1)), ("gw * gh wraps 32 bits", put(p + 1, 0xffffffff)),
            ("factor 0", put(p + 2, 0)), ("fill 0", put(p + 3, 0)), ("fill 9", put(p + 3, 9)),
            ("offset below 192", put(p + 6, 188)), ("offset 128", put(p + 6, 128)), ("offset 0", put(p + 6, 0)), ("offset odd", put(p + 6, w[p + 6] + 2)),
            ("offset past the end", put(p + 6, w[p + 6] + 4)), ("offset huge", put(p + 6, 0xfffffffc)),
            ("array past the end", put(p + 1, w[p + 1] + 1))]
    for k in range(12):
        out += [("camera word %d %s" % (k, name), put(32 + k, bits(v))) for name, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf))]
    out += [("singular: W = U", struct.pack("<48I", *(w[:41] + w[35:38] + w[44:])) + body),
            ("singular: V = 0", struct.pack("<48I", *(w[:38] + [0, 0, 0] + w[41:])) + body),
            ("near 0", put(44, 0)), ("near -0", put(44, bits(-0.0))), ("near negative", put(44, bits(-0.1))), ("near nan", put(44, bits(np.nan))),
            ("near inf", put(44, bits(np.inf))), ("word 45", put(45, 1)), ("word 46", put(46, 1 << 31)), ("word 47", put(47, 7))]
    return out
