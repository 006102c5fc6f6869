"""ctypes mirrors of the depth packet's structures (include/fovpt.h, fovpt_packet_depth_*), pinned to the compiled header by
tests/test_packet_depth_cpu.py."""
import ctypes as C

from . import abi

PACKET_MAGIC_DEPTH = 0x44505646                 # FOVPT_PACKET_MAGIC_DEPTH, "FVPD"
PACKET_DEPTH_HEADER_BYTES = 192                 # FOVPT_PACKET_DEPTH_HEADER_BYTES


class PacketDepthConfig(abi.Struct):
    """fovpt_packet_depth_config: the depth below which a depth packet's codes saturate (defaults: fovpt_packet_depth_defaults)."""
    _fields_ = [("near", C.c_float), ("_reserved", C.c_uint32 * 3)]


class PacketDepthHeader(abi.Struct):
    """fovpt_packet_depth_header: the first 192 bytes of a depth packet ("FVPD") -- a packet header whose pass records are those
    of the frame's colour packet, the camera the frame was rendered with, and near."""
    _fields_ = [("base", abi.PacketHeader), ("camera", abi.WarpCamera), ("near", C.c_float), ("_reserved", C.c_uint32 * 3)]

    @classmethod
    def from_packet(cls, data):
        """The header of a depth packet's bytes (unchecked: fovpt_packet_check_depth checks)."""
        return cls.from_buffer_copy(bytes(data[:C.sizeof(cls)]))
