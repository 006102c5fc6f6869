"""fovpt_packet_* on the GPU against tests/packet_ref.py, byte for byte: the encoder on rendered frames and on uploaded images,
the round trip through the device decoder and the host decoder, the slots and their ordering with frames in flight, the buffers
the calls must leave alone, every rejection of the context's entry points, a seeded sweep and the C++ drop-in.  The scene is the
Cornell box at the shapes of tests/packet_cases.py, spp 1 / 1 / 2."""
import ctypes as C
import os

import numpy as np
import pytest

import packet_ref as pk
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import build_dropin, device_filled, dropin_renderer, run_dropin, upload
from packet_cases import IDS, JUNK, SHAPES, junk_canvas, mutations, random_frame

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_FRAME = -1, -5
PROBE = scenes.ambient_probe(64, 32, 2.0)


def _cornell(size, gaze, radii, uniform, spp=(1, 1, 2), guides=False):
    cfg = cfg_uniform(1) if uniform else cfg_foveated(radii[0], radii[1], spp)
    cfg.write_guides = 1 if guides else 0
    return make_gpu(scenes.cornell_box(), PROBE, scenes.CORNELL_CAMERA, size, cfg, gaze=gaze)


def frame_of(r):
    """(size, gaze, radii, FOV_OFF) of the frame r rendered last, as packet_ref takes them."""
    f, cfg = r.launchParams.frame, r.config
    return (f.size.x, f.size.y), (f.c.x, f.c.y), (cfg.r_inner, cfg.r_outer), bool(cfg.uniform)


def encode_on_device(r, sequence, in_rgba=None):
    """fovpt_packet_encode into a junk-filled buffer 64 bytes longer than the packet -> the packet's bytes; the tail stays junk."""
    h = r.describePacket(sequence)
    buf = device_filled(h.bytes + 64)
    h2 = r.encodePacket(buf.data_ptr(), sequence, in_rgba)
    assert bytes(h) == bytes(h2)
    r.synchronize()
    got = buf.cpu().numpy().tobytes()
    assert got[h.bytes:] == bytes([0x5a]) * 64
    assert got[:128] == bytes(h)
    return got[:h.bytes], buf


def decode_on_device(r, packet_dev, header, mode):
    size = (header.width, header.height)
    out = upload(junk_canvas(size))
    r.decodePacket(header, packet_dev.data_ptr(), out.data_ptr(), mode)
    r.synchronize()
    return out.cpu().numpy().view(np.uint32)


def host_decode(packet, mode, size):
    return renderer.decode_packet(packet, mode, size, out=junk_canvas(size))


# ---- 6. the encoder against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_encode_matches_the_reference_byte_for_byte(shape):
    size, gaze, radii, uniform = shape
    r = _cornell(size, gaze, radii, uniform)
    r.render()
    frame = r.downloadPixels()
    got, _ = encode_on_device(r, 41)
    want = pk.encode(frame, *frame_of(r), sequence=41)
    assert len(got) == len(want) and got == want
    assert len(np.unique(np.frombuffer(got, np.uint32, offset=128))) > 4       # (a picture, zeros among it where a texel owns nothing)
    img = random_frame(size, 5)
    dev = upload(img)
    got, _ = encode_on_device(r, 0xfffffff0, dev.data_ptr())
    assert got == pk.encode(img, *frame_of(r), sequence=0xfffffff0)
    odd = upload(np.concatenate([np.zeros(1, np.uint32), img.reshape(-1)]))   # an input that is only 4-byte aligned
    got, _ = encode_on_device(r, 7, odd.data_ptr() + 4)
    assert got == pk.encode(img, *frame_of(r), sequence=7)
    r.close()


# ---- 7. the round trip ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_round_trip_device_and_host(shape):
    size, gaze, radii, uniform = shape
    r = _cornell(size, gaze, radii, uniform)
    r.render()
    frame = r.downloadPixels()
    written = pk.owners(*frame_of(r))[0] >= 0
    assert written.any()
    packet, dev = encode_on_device(r, 1)
    h = abi.PacketHeader.from_packet(packet)
    got = decode_on_device(r, dev, h, abi.PACKET_NEAREST)
    assert np.array_equal(got[written], frame[written]) and (got[~written] == JUNK).all()      # no pixel excluded
    assert np.array_equal(host_decode(packet, abi.PACKET_NEAREST, size), got)
    img = random_frame(size, 6)
    keep = upload(img)
    packet, dev = encode_on_device(r, 2, keep.data_ptr())
    for mode in (abi.PACKET_NEAREST, abi.PACKET_SMOOTH):
        want = pk.decode(packet, mode, junk_canvas(size))
        got = decode_on_device(r, dev, h, mode)
        assert np.array_equal(got, want), (mode, int((got != want).sum()))
        assert np.array_equal(host_decode(packet, mode, size), want), mode
    r.close()


# ---- 8. slots and ordering ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "frames_in_flight", "chains_per_frame"])
def test_slots_and_ordering(mode):
    """Six frames with a gaze that moves every frame, each submitted as a packet with the next frame rendered at once and no
    synchronisation: every wait returns the packet of its own frame."""
    if mode == "default":
        size, radii, spp = (64, 48), (6, 14), (1, 1, 2)
    else:
        size, radii, spp = (384, 216), (20, 60), (4, 8, 16)      # >= 16384 sample slots: chains_per_frame = 2 does split the frame
    r = _cornell(size, (size[0] // 2, size[1] // 2), radii, False, spp)
    cfg = r.config
    if mode == "frames_in_flight":
        cfg.frames_in_flight = 2
    elif mode == "chains_per_frame":
        cfg.chains_per_frame = 2
    r.config = cfg
    views = [((size[0] // 2 + 17 * k) % size[0], (size[1] // 3 + 11 * k) % size[1]) for k in range(6)]

    def setup(k):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = views[k]
        r.launchParams.frame.subframe_index = k

    want = []
    for k in range(6):                                       # the frames one by one: what the packets must be
        setup(k)
        r.render()
        want.append(pk.encode(r.downloadPixels(), *frame_of(r), sequence=1000 + k))
    assert len(set(want)) == 6
    slots, got = [], {}
    for k in range(6):
        setup(k)
        r.render_async()
        slots.append(r.submitPacket(1000 + k))
        if k >= 2:                                           # the slot submitted two frames earlier, while frames k - 1 and k run
            got[k - 2] = r.waitPacket(slots[k - 2])
    assert slots == [0, 1, 2, 3, 0, 1]                       # after four submits the fifth reuses slot 0
    for k in (4, 5):
        got[k] = r.waitPacket(slots[k])
    for k in range(6):
        assert abi.PacketHeader.from_packet(got[k]).sequence == 1000 + k
        assert got[k] == want[k], k
    assert r.waitPacket(2) == want[2] and r.waitPacket(3) == want[3]      # finished slots stay readable, as often as asked
    # ... also across fovpt_resize and fovpt_set_scene
    r.resize((40, 24))
    assert r.waitPacket(1) == want[5]
    from test_temporal_gpu import _scene_again
    _scene_again(r)
    assert r.waitPacket(0) == want[4]
    r.close()


# ---- 9. side effects ------------------------------------------------------------------------------------------------------------------
def test_encode_and_submit_leave_every_other_buffer_alone():
    size = (96, 64)
    r = _cornell(size, (40, 30), (10, 24), False, (1, 2, 4), guides=True)
    r.render()
    r.denoise()
    r.reconstruct()
    r.temporal()
    r.post()
    r.expose(None, r.post_buffers()[0])

    def snapshot():
        return [x.tobytes() for x in (r.downloadPixels(), r.downloadAccum(), r.downloadDenoisedColor(), r.downloadDenoisedPixels(), r.downloadPostColor(),
                                      r.downloadPostPixels(), r.downloadExposedColor(), r.downloadExposedPixels(), r.downloadTemporalHistory())]

    before = snapshot()
    packets = []
    for k, src in enumerate((None, r.post_buffers()[1], r.expose_buffers()[1], r.denoise_buffers()[1])):
        packets.append(encode_on_device(r, k, src)[0])
        assert r.waitPacket(r.submitPacket(k, src)) == packets[-1]
    assert snapshot() == before
    assert len(set(packets)) == 4
    exposed = np.frombuffer(before[7], np.uint32).reshape(size[1], size[0])
    assert packets[2] == pk.encode(exposed, *frame_of(r), sequence=2)
    r.close()


# ---- 10. rejections -------------------------------------------------------------------------------------------------------------------
def test_rejections_all_or_nothing():
    L = lib.load()
    size, gaze, radii, uniform = SHAPES[0]
    r = _cornell(size, gaze, radii, uniform)
    lp = C.byref(r.launchParams)
    hdr, slot, ptr, n = abi.PacketHeader(), C.c_int(-7), C.c_void_p(), C.c_size_t()
    buf = device_filled(4096)

    def untouched():
        r.synchronize()
        return (buf.cpu().numpy() == 0x5a).all() and slot.value == -7

    # nothing rendered yet
    assert L.fovpt_packet_describe(r._ctx, lp, 0, C.byref(hdr)) == E_NO_FRAME
    assert L.fovpt_packet_encode(r._ctx, lp, None, 0, buf.data_ptr()) == E_NO_FRAME
    assert L.fovpt_packet_submit(r._ctx, lp, None, 0, C.byref(slot)) == E_NO_FRAME
    for s in range(-1, 6):
        assert L.fovpt_packet_wait(r._ctx, s, C.byref(ptr), C.byref(n)) == E_INVALID      # out of range, or never submitted
    r.render()
    # null arguments
    assert L.fovpt_packet_describe(None, lp, 0, C.byref(hdr)) == E_INVALID and L.fovpt_packet_describe(r._ctx, None, 0, C.byref(hdr)) == E_INVALID
    assert L.fovpt_packet_describe(r._ctx, lp, 0, None) == E_INVALID
    assert L.fovpt_packet_encode(None, lp, None, 0, buf.data_ptr()) == E_INVALID and L.fovpt_packet_encode(r._ctx, None, None, 0, buf.data_ptr()) == E_INVALID
    assert L.fovpt_packet_encode(r._ctx, lp, None, 0, None) == E_INVALID
    assert L.fovpt_packet_submit(None, lp, None, 0, C.byref(slot)) == E_INVALID and L.fovpt_packet_submit(r._ctx, None, None, 0, C.byref(slot)) == E_INVALID
    assert L.fovpt_packet_submit(r._ctx, lp, None, 0, None) == E_INVALID
    assert L.fovpt_packet_wait(None, 0, C.byref(ptr), C.byref(n)) == E_INVALID and L.fovpt_packet_wait(r._ctx, 0, None, C.byref(n)) == E_INVALID
    assert L.fovpt_packet_wait(r._ctx, 0, C.byref(ptr), None) == E_INVALID
    # another frame size; a null frame buffer
    f = r.launchParams.frame
    f.size.x -= 4
    assert L.fovpt_packet_encode(r._ctx, lp, None, 0, buf.data_ptr()) == E_NO_FRAME and L.fovpt_packet_submit(r._ctx, lp, None, 0, C.byref(slot)) == E_NO_FRAME
    assert L.fovpt_packet_describe(r._ctx, lp, 0, C.byref(hdr)) == E_NO_FRAME
    f.size.x += 4
    keep = f.frame_buffer
    f.frame_buffer = None
    assert L.fovpt_packet_encode(r._ctx, lp, None, 0, buf.data_ptr()) == E_NO_FRAME and L.fovpt_packet_submit(r._ctx, lp, None, 0, C.byref(slot)) == E_NO_FRAME
    f.frame_buffer = keep
    assert untouched()
    # a tile shard does not see the frame
    c = r.config
    c.world, c.rank = 2, 0
    r.config = c
    r.render()
    assert L.fovpt_packet_describe(r._ctx, lp, 0, C.byref(hdr)) == E_INVALID and L.fovpt_packet_encode(r._ctx, lp, None, 0, buf.data_ptr()) == E_INVALID
    assert L.fovpt_packet_submit(r._ctx, lp, None, 0, C.byref(slot)) == E_INVALID
    assert b"world" in L.fovpt_last_error(r._ctx)
    c.world, c.rank = 1, 0
    r.config = c
    r.render()
    assert untouched()
    # the decoder: null arguments, modes, and every header fovpt_packet_check refuses
    packet, dev = encode_on_device(r, 3)
    good = abi.PacketHeader.from_packet(packet)
    out = upload(junk_canvas(size))
    args = (C.byref(good), dev.data_ptr(), 0, out.data_ptr())
    assert L.fovpt_packet_decode(None, *args) == E_INVALID
    for k in (0, 1, 3):
        a = list(args)
        a[k] = None
        assert L.fovpt_packet_decode(r._ctx, *a) == E_INVALID, k
    for m in (-1, 2, 77):
        assert L.fovpt_packet_decode(r._ctx, C.byref(good), dev.data_ptr(), m, out.data_ptr()) == E_INVALID
    refused = 0
    for label, m in mutations(packet):
        if label.startswith(("another", "bytes above")):     # (valid headers: the device decoder has no output size and no byte count to hold them against)
            continue
        bad = abi.PacketHeader.from_packet(m)
        assert L.fovpt_packet_decode(r._ctx, C.byref(bad), dev.data_ptr(), 0, out.data_ptr()) == E_INVALID, label
        refused += 1
    assert refused == len(mutations(packet)) - 3 >= 25      # (all but "another width", "another height" and "bytes above")
    far = abi.PacketHeader.from_packet(packet)               # a pass that reaches beyond the device decoder's search
    far.passes[0].factor = 1 << 28
    assert pk.check(bytes(far) + packet[128:]) and L.fovpt_packet_decode(r._ctx, C.byref(far), dev.data_ptr(), 0, out.data_ptr()) == E_INVALID
    r.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == JUNK).all()
    # none of the refused submits took a slot; the valid calls after them
    assert r.submitPacket(9) == 0 and r.submitPacket(10) == 1
    assert abi.PacketHeader.from_packet(r.waitPacket(1)).sequence == 10 and r.waitPacket(0)[128:] == packet[128:]
    assert L.fovpt_packet_wait(r._ctx, 2, C.byref(ptr), C.byref(n)) == E_INVALID
    r.close()


# ---- 11. a seeded sweep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("FOVPT_FUZZP_TO", "8"))))
def test_seeded_sweep(seed):
    rng = np.random.default_rng(4000 + seed)
    w, h = int(rng.integers(4, 97)), int(rng.integers(4, 81))      # (a side below 4 has no periphery launch index: no packet)
    uniform = bool(rng.random() < 0.25)
    ri = int(rng.integers(0, 12))
    radii = (ri, ri + int(rng.integers(0, 24)))
    gaze = (int(rng.integers(-8, w + 8)) & 0xffffffff, int(rng.integers(-8, h + 8)) & 0xffffffff)
    r = _cornell((w, h), gaze, radii, uniform, (1, 1, 1))
    r.render()
    frame = r.downloadPixels()
    fr = frame_of(r)
    written = pk.owners(*fr)[0] >= 0
    packet, dev = encode_on_device(r, seed)
    assert packet == pk.encode(frame, *fr, sequence=seed), (seed, fr)
    hd = abi.PacketHeader.from_packet(packet)
    got = decode_on_device(r, dev, hd, abi.PACKET_NEAREST)
    assert np.array_equal(got[written], frame[written]) and (got[~written] == JUNK).all(), (seed, fr)
    img = random_frame((w, h), seed)
    keep = upload(img)
    packet, dev = encode_on_device(r, seed + 1, keep.data_ptr())
    assert packet == pk.encode(img, *fr, sequence=seed + 1), (seed, fr)
    assert r.waitPacket(r.submitPacket(seed + 1, keep.data_ptr())) == packet
    for mode in (abi.PACKET_NEAREST, abi.PACKET_SMOOTH):
        want = pk.decode(packet, mode, junk_canvas((w, h)))
        assert np.array_equal(decode_on_device(r, dev, hd, mode), want), (seed, fr, mode)
        assert np.array_equal(host_decode(packet, mode, (w, h)), want), (seed, fr, mode)
    r.close()


# ---- 12. the C++ drop-in --------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_packets(tmp_path):
    """SampleRenderer::submitPacket() / waitPacket() of include/SimplePathtracer.h and fovpt_packet_decode_host: three frames in
    flight, each packet decoded on the host and compared with downloadPixels -- there and, with the reference, here."""
    exe, out = build_dropin(tmp_path, "packet_gpu_test"), str(tmp_path / "packet_out.bin")
    run_dropin(exe, out)
    size, n = (160, 96), 160 * 96
    raw = np.fromfile(out, np.uint32)
    sizes, frames, decoded = raw[:3], raw[3:3 + 3 * n].reshape(3, 96, 160), raw[3 + 3 * n:].reshape(3, 96, 160)
    for k, gaze in enumerate([(80, 48), (150, 10), (3, 90)]):
        packet = pk.encode(frames[k], size, gaze, (12, 36), False, sequence=100 + k)
        assert sizes[k] == len(packet)
        assert np.array_equal(pk.decode(packet, pk.NEAREST, np.zeros((96, 160), np.uint32)), decoded[k]), k
        written = pk.owners(size, gaze, (12, 36), False)[0] >= 0
        assert np.array_equal(decoded[k][written], frames[k][written]) and not decoded[k][~written].any() and written.mean() > 0.99
        assert len(np.unique(decoded[k])) > 20
    # the frames are what Python renders
    r = dropin_renderer(gaze=(150, 10), subframe_index=1)
    r.render()
    written = pk.owners(size, (150, 10), (12, 36), False)[0] >= 0
    assert np.array_equal(r.downloadPixels()[written], frames[1][written])
    r.close()
