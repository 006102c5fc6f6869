"""What the packet tests on the CPU and on the GPU share: the shapes, the input frames and the one-field mutations."""
import struct

import numpy as np

import packet_ref as pk

# (size, gaze, radii, FOV_OFF)
SHAPES = [
    ((64, 48), (32, 24), (6, 14), False),
    ((64, 48), (62, 46), (6, 14), False),          # the folded last column / row
    ((64, 48), (0, 0), (6, 14), False),            # wrapped offsets
    ((66, 50), (65, 49), (6, 14), False),          # sizes that are no multiple of 4: pixels nobody writes
    ((67, 49), (3, 47), (5, 13), False),
    ((33, 21), (16, 10), None, True),
]
IDS = ["%dx%d-%s" % (s[0], s[1], "fov_off" if u else "g%d.%d" % g) for s, g, r, u in SHAPES]
JUNK = np.uint32(0x5a17c3e9)                      # (alpha 0x5a: a value no frame and no texel holds)


def random_frame(size, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, (size[1], size[0]), dtype=np.uint64).astype(np.uint32)


def synthetic_raw(size, gaze, radii, uniform, seed=0):
    """A frame as the resolve leaves it: every written pixel a function of its writer (alpha 0xff), junk where nothing writes.
    -> (frame, written mask)."""
    own_p, own_l = pk.owners(size, gaze, radii, uniform)
    v = ((own_p + 1) * 2654435761 + own_l * 40503 + seed * 97) & 0xffffff
    written = own_p >= 0
    return np.where(written, v | 0xff000000, int(JUNK)).astype(np.uint32), written


def junk_canvas(size):
    return np.full((size[1], size[0]), JUNK, np.uint32)


def mutations(packet):
    """(label, mutated packet) for every rejection fovpt_packet_check lists: one field of a valid packet changed each."""
    w = list(struct.unpack("<32I", packet[:128]))
    npass = w[6]
    body = packet[128:]

    def put(i, v):
        m = list(w)
        m[i] = v & 0xffffffff
        return struct.pack("<32I", *m) + body

    out = [("magic", put(0, w[0] ^ 1)), ("version 0", put(1, 0)), ("version 2", put(1, 2)),
           ("bytes above the bytes given", put(2, w[2] + 4)), ("bytes below 128", put(2, 124)), ("bytes 0", put(2, 0)),
           ("width 0", put(4, 0)), ("width -1", put(4, -1)), ("width 16385", put(4, 16385)), ("another width", put(4, w[4] + 1)),
           ("height 0", put(5, 0)), ("height 16385", put(5, 16385)), ("another height", put(5, w[5] - 1)),
           ("npass 0", put(6, 0)), ("npass 4", put(6, 4)), ("reserved", put(7, 1))]
    if npass < 3:
        out += [("npass + 1 over a zero entry", put(6, npass + 1))]
        out += [("unused pass entry word %d" % k, put(8 + 8 * npass + k, 1)) for k in range(8)]
    p = 8 + 8 * (npass - 1)                       # the last pass
    out += [("pass reserved", put(p + 7, 1)), ("gw 0", put(p + 0, 0)), ("gh 0", put(p + 1, 0)),
            ("too many texels", put(p + 1, (1 << 26) // w[p + 0] + 1)), ("gw * gh wraps 32 bits", put(p + 1, 0xffffffff)),
            ("factor 0", put(p + 2, 0)), ("fill 0", put(p + 3, 0)), ("fill 9", put(p + 3, 9)),
            ("offset below 128", put(p + 6, 124)), ("offset 0", put(p + 6, 0)), ("offset odd", put(p + 6, w[p + 6] + 2)),
            ("offset past the end", put(p + 6, w[p + 6] + 4)), ("offset huge", put(p + 6, 0xfffffffc)),
            ("array past the end", put(p + 1, w[p + 1] + 1))]
    return out
