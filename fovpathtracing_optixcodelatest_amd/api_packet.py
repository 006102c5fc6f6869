"""The foveated frame packets of SampleRenderer, beside csrc/api_packet.hip (decode_packet, the client's side, is in renderer.py)."""
import ctypes as C

from . import abi, abi_depth


class Packets:
    """Mixed into SampleRenderer (renderer.py), which brings _L, _ctx, _check and launchParams."""

    # -- foveated frame packets (include/fovpt.h, fovpt_packet_*): a frame off the device, small and without stopping the renderer
    def packetConfig(self, codec=True) -> abi.PacketConfig:
        """The fovpt_packet_config of a codec= argument: True -> fovpt_packet_defaults (BC1 where a pass's fill is above 1), a
        sequence of up to three abi.PACKET_RAW / PACKET_BC1 / PACKET_BY_FILL -> those, per launch pass; an abi.PacketConfig as it is."""
        if isinstance(codec, abi.PacketConfig):
            return codec
        cfg = abi.PacketConfig()
        self._L.fovpt_packet_defaults(C.byref(cfg))
        if codec is not True:
            codec = [int(k) for k in codec]
            if len(codec) > 3:
                raise ValueError("codec: at most three passes")
            for p in range(3):
                cfg.codec[p] = codec[p] if p < len(codec) else 0
        return cfg

    def describePacket(self, sequence=0, codec=None) -> abi.PacketHeader:
        """The header encodePacket / submitPacket would write for the frame last rendered (host only); .bytes sizes a buffer.
        codec: None -> a raw "FVPK" packet; otherwise a coded "FVPC" one (packetConfig)."""
        h = abi.PacketHeader()
        if codec is None:
            self._check(self._L.fovpt_packet_describe(self._ctx, C.byref(self.launchParams), sequence, C.byref(h)))
        else:
            self._check(self._L.fovpt_packet_describe_coded(self._ctx, C.byref(self.launchParams), C.byref(self.packetConfig(codec)), sequence, C.byref(h)))
        return h

    def encodePacket(self, out_packet, sequence=0, in_rgba=None, codec=None) -> abi.PacketHeader:
        """Encodes the frame last rendered into out_packet, a device pointer with describePacket().bytes of room.  in_rgba: device
        pointer of an rgba8 image of the frame's size (post_buffers()[1], expose_buffers()[1], ...), None: the frame buffer.
        Enqueued on the renderer's stream, not synchronised.  Returns the header it writes."""
        h = self.describePacket(sequence, codec)
        if codec is None:
            self._check(self._L.fovpt_packet_encode(self._ctx, C.byref(self.launchParams), in_rgba, sequence, out_packet))
        else:
            self._check(self._L.fovpt_packet_encode_coded(self._ctx, C.byref(self.launchParams), C.byref(self.packetConfig(codec)), in_rgba, sequence, out_packet))
        return h

    def submitPacket(self, sequence=0, in_rgba=None, codec=None) -> int:
        """encodePacket into the next of abi.PACKET_SLOTS slots and an asynchronous copy to the slot's pinned host buffer: does
        not wait for the GPU (except for the slot's previous copy, if that is still running).  Returns the slot for waitPacket."""
        slot = C.c_int(-1)
        if codec is None:
            self._check(self._L.fovpt_packet_submit(self._ctx, C.byref(self.launchParams), in_rgba, sequence, C.byref(slot)))
        else:
            self._check(self._L.fovpt_packet_submit_coded(self._ctx, C.byref(self.launchParams), C.byref(self.packetConfig(codec)), in_rgba, sequence, C.byref(slot)))
        return slot.value

    def waitPacket(self, slot) -> bytes:
        """Waits for that slot's copy alone (later frames keep running) and returns the packet's bytes: what a client hands to
        decode_packet()."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.fovpt_packet_wait(self._ctx, slot, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value)

    def decodePacket(self, header, packet, out_rgba, mode=abi.PACKET_NEAREST):
        """The device decoder: header an abi.PacketHeader (host), packet and out_rgba device pointers (out_rgba: the header's
        width x height rgba8 pixels; those no texel reaches keep their contents).  Enqueued on the renderer's stream."""
        self._check(self._L.fovpt_packet_decode(self._ctx, C.byref(header), packet, int(mode), out_rgba))

    # -- depth packets (include/fovpt.h, fovpt_packet_*_depth): the frame's depth and camera, for a client that warps (api_post.warp_depth)
    def depthPacketConfig(self, near=None) -> abi_depth.PacketDepthConfig:
        """The fovpt_packet_depth_config of a near= argument: None -> fovpt_packet_depth_defaults, a number -> that near; an
        abi_depth.PacketDepthConfig as it is."""
        if isinstance(near, abi_depth.PacketDepthConfig):
            return near
        cfg = abi_depth.PacketDepthConfig()
        self._L.fovpt_packet_depth_defaults(C.byref(cfg))
        if near is not None:
            cfg.near = near
        return cfg

    def describeDepthPacket(self, sequence=0, near=None) -> abi_depth.PacketDepthHeader:
        """The header encodeDepthPacket / submitDepthPacket would write for the frame last rendered (host only); .base.bytes
        sizes a buffer."""
        h = abi_depth.PacketDepthHeader()
        self._check(self._L.fovpt_packet_describe_depth(self._ctx, C.byref(self.launchParams), C.byref(self.depthPacketConfig(near)), sequence, C.byref(h)))
        return h

    def encodeDepthPacket(self, out_packet, sequence=0, gbuffer=None, near=None) -> abi_depth.PacketDepthHeader:
        """Encodes the depth of the frame last rendered into out_packet, a device pointer with describeDepthPacket().base.bytes
        of room.  gbuffer: an abi.GBufferPtrs of the rendered frame (temporal_gbuffer() saves the trace), None: traced by the
        call.  Enqueued on the renderer's stream, not synchronised.  Returns the header it writes."""
        h = self.describeDepthPacket(sequence, near)
        self._check(self._L.fovpt_packet_encode_depth(self._ctx, C.byref(self.launchParams), C.byref(self.depthPacketConfig(near)),
                                                      C.byref(gbuffer) if gbuffer is not None else None, sequence, out_packet))
        return h

    def submitDepthPacket(self, sequence=0, gbuffer=None, near=None) -> int:
        """encodeDepthPacket into the next of the slots submitPacket uses, and the asynchronous copy to the host.  Returns the
        slot for waitPacket."""
        slot = C.c_int(-1)
        self._check(self._L.fovpt_packet_submit_depth(self._ctx, C.byref(self.launchParams), C.byref(self.depthPacketConfig(near)),
                                                      C.byref(gbuffer) if gbuffer is not None else None, sequence, C.byref(slot)))
        return slot.value

    def decodeDepthPacket(self, header, packet, out_depth):
        """The device decoder of a depth packet: header an abi_depth.PacketDepthHeader (host), packet and out_depth device
        pointers (out_depth: the header's width x height floats, +inf the sky; those no texel reaches keep their contents).
        Needs no scene and no rendered frame.  Enqueued on the renderer's stream."""
        self._check(self._L.fovpt_packet_decode_depth(self._ctx, C.byref(header), packet, out_depth))
