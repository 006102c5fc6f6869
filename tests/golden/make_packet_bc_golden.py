"""Writes tests/golden/packet_c1_64x48.bin (1136 bytes: the frame of packet_v1_64x48.bin as a coded packet, P and M as BC1 blocks,
the fovea raw) and its two decoded images from tests/packet_bc_ref.py: the coded wire format, pinned.  Run from the repository
root: python tests/golden/make_packet_bc_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import packet_bc_ref as bc                                   # noqa: E402
import packet_ref as pk                                      # noqa: E402
from packet_cases import SHAPES, random_frame                # noqa: E402

size, gaze, radii, uniform = SHAPES[0]
packet = bc.encode(random_frame(size, 2024), size, gaze, radii, uniform, sequence=0x01020304)
assert len(packet) == 1136
open(os.path.join(HERE, "packet_c1_64x48.bin"), "wb").write(packet)
for mode, name in ((pk.NEAREST, "nearest"), (pk.SMOOTH, "smooth")):
    bc.decode(packet, mode, np.zeros((size[1], size[0]), np.uint32)).astype("<u4").tofile(os.path.join(HERE, "packet_c1_64x48_%s.bin" % name))
