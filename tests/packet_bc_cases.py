"""What the coded-packet tests on the CPU and on the GPU share: the codec masks and the one-field mutations of a coded packet."""
import struct

import packet_bc_ref as bc
from packet_cases import mutations

MASKS = [(1, 1, 1), (1, 1, 0), (0, 1, 0), (0, 0, 0)]


def masks_for(npass):
    """The masks cut to a frame's passes, each once (FOV_OFF: (1,) and (0,))."""
    out = []
    for m in MASKS:
        if m[:npass] not in out:
            out.append(m[:npass])
    return out


def coded_mutations(packet):
    """(label, mutated packet) for every rejection of a coded packet: those of packet_cases.mutations whose meaning the codec word
    does not change, and the codec's own."""
    w = list(struct.unpack("<32I", packet[:128]))
    npass = w[6]
    body = packet[128:]

    def put(i, v):
        m = list(w)
        m[i] = v & 0xffffffff
        return struct.pack("<32I", *m) + body

    # ("pass reserved" = 1 is a codec here; "array past the end" adds one texel row, which a BC1 pass may hold already)
    out = [(label, m) for label, m in mutations(packet) if label not in ("pass reserved", "array past the end")]
    p = 8 + 8 * (npass - 1)                       # the last pass: its array ends where the packet does
    out += [("codec 2", put(p + 7, 2)), ("codec -1", put(p + 7, -1)), ("codec 1 << 8", put(p + 7, 256)), ("codec 2 in pass 0", put(15, 2))]
    if w[p + 7] == bc.BC1:
        out += [("array past the end by one block row", put(p + 1, 4 * ((w[p + 1] + 3) // 4) + 1)),
                ("array past the end by one block column", put(p + 0, 4 * ((w[p + 0] + 3) // 4) + 1)),
                ("array past bytes by one block", struct.pack("<32I", *(w[:2] + [w[2] - 8] + w[3:])) + body[:-8])]
    else:
        out += [("array past the end", put(p + 1, w[p + 1] + 1)),
                ("array past bytes by one texel", struct.pack("<32I", *(w[:2] + [w[2] - 4] + w[3:])) + body[:-4])]
    return out
