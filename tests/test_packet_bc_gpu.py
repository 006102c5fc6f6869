"""Coded frame packets on the GPU against tests/packet_bc_ref.py, byte for byte: k_packet_encode_coded on rendered frames and on
uploaded images for every codec mask, the device decoder's CODED instantiations in both modes, the round trip, raw and coded
submits alternating over the slots, the error codes, a seeded sweep, and the raw encoder as it was.  The scene is the Cornell
box at the shapes of tests/packet_cases.py, spp 1 / 1 / 2."""
import ctypes as C
import os

import numpy as np
import pytest

import packet_bc_ref as bc
import packet_ref as pk
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer, scenes

from common import cfg_foveated, cfg_uniform, make_gpu
from gpu_common import device_filled, upload
from packet_bc_cases import coded_mutations, masks_for
from packet_cases import IDS, JUNK, SHAPES, junk_canvas, random_frame

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_FRAME = -1, -5
PROBE = scenes.ambient_probe(64, 32, 2.0)
CANARY = 64
# ... and an 8 x 8 frame whose periphery grid (2 x 2) is smaller than one block
ALL_SHAPES = SHAPES + [((8, 8), (5, 5), (0, 1), False)]
ALL_IDS = IDS + ["8x8-g5.5"]


def _cornell(size, gaze, radii, uniform, spp=(1, 1, 2)):
    cfg = cfg_uniform(1) if uniform else cfg_foveated(radii[0], radii[1], spp)
    return make_gpu(scenes.cornell_box(), PROBE, scenes.CORNELL_CAMERA, size, cfg, gaze=gaze)


def frame_of(r):
    """(size, gaze, radii, FOV_OFF) of the frame r rendered last, as packet_ref takes them."""
    f, cfg = r.launchParams.frame, r.config
    return (f.size.x, f.size.y), (f.c.x, f.c.y), (cfg.r_inner, cfg.r_outer), bool(cfg.uniform)


def encode_on_device(r, sequence, codec, in_rgba=None):
    """fovpt_packet_encode_coded into a junk-filled buffer with canary bytes behind the packet -> (the packet's bytes, the device
    buffer); the canary stays."""
    h = r.describePacket(sequence, codec)
    buf = device_filled(h.bytes + CANARY)
    h2 = r.encodePacket(buf.data_ptr(), sequence, in_rgba, codec)
    assert bytes(h) == bytes(h2)
    r.synchronize()
    got = buf.cpu().numpy().tobytes()
    assert got[h.bytes:] == bytes([0x5a]) * CANARY
    assert got[:128] == bytes(h)
    return got[:h.bytes], buf


def decode_on_device(r, packet_dev, header, mode):
    out = upload(junk_canvas((header.width, header.height)))
    r.decodePacket(header, packet_dev.data_ptr(), out.data_ptr(), mode)
    r.synchronize()
    return out.cpu().numpy().view(np.uint32)


# ---- the encoder and the decoder against the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=ALL_IDS)
def test_encode_and_decode_match_the_reference(shape):
    size, gaze, radii, uniform = shape
    r = _cornell(size, gaze, radii, uniform)
    r.render()
    frame = r.downloadPixels()
    fr = frame_of(r)
    own = pk.owners(*fr)[0]
    written = own >= 0
    npass = len(pk.passes(*fr))
    img = random_frame(size, 5)
    dev = upload(img)                                                     # 16-byte aligned: the row path where the width allows
    odd = upload(np.concatenate([np.zeros(1, np.uint32), img.reshape(-1)]))   # only 4-byte aligned: the scalar path
    raw_packet = pk.encode(frame, *fr, sequence=41)
    for mask in masks_for(npass):
        got, buf = encode_on_device(r, 41, mask)
        want = bc.encode(frame, *fr, mask, sequence=41)
        assert len(got) == len(want) and got == want, mask
        assert want == bc.transcode(raw_packet, mask)
        hd = abi.PacketHeader.from_packet(got)
        assert hd.magic == abi.PACKET_MAGIC_CODED and [hd.passes[p]._reserved for p in range(npass)] == list(mask)
        for mode in (abi.PACKET_NEAREST, abi.PACKET_SMOOTH):
            ref = bc.decode(want, mode, junk_canvas(size))
            dec = decode_on_device(r, buf, hd, mode)
            assert np.array_equal(dec, ref), (mask, mode, int((dec != ref).sum()))
            assert np.array_equal(dec != JUNK, written), (mask, mode)     # exactly the raw frame's written pixel set
            if mode == abi.PACKET_NEAREST and npass == 3 and mask[2] == 0:
                assert ((own == 2).any() or size == (8, 8)) and np.array_equal(dec[own == 2], frame[own == 2])      # the fovea raw: exact
        got, buf = encode_on_device(r, 0xfffffff0, mask, dev.data_ptr())
        want = bc.encode(img, *fr, mask, sequence=0xfffffff0)
        assert got == want, mask
        for mode in (abi.PACKET_NEAREST, abi.PACKET_SMOOTH):
            ref = bc.decode(want, mode, junk_canvas(size))
            dec = decode_on_device(r, buf, hd, mode)
            assert np.array_equal(dec, ref), (mask, mode, int((dec != ref).sum()))
            assert np.array_equal(renderer.decode_packet(got, mode, size, out=junk_canvas(size)), ref)
        got, _ = encode_on_device(r, 7, mask, odd.data_ptr() + 4)
        assert got == bc.encode(img, *fr, mask, sequence=7), mask
    # the defaults: BC1 where the fill is above 1
    got, _ = encode_on_device(r, 3, True)
    assert got == bc.encode(frame, *fr, None, sequence=3)
    assert [abi.PacketHeader.from_packet(got).passes[p]._reserved for p in range(npass)] == ([0] if uniform else [1, 1, 0])
    # the raw encoder, as it was
    h = r.describePacket(9)
    buf = device_filled(h.bytes + CANARY)
    r.encodePacket(buf.data_ptr(), 9, dev.data_ptr())
    r.synchronize()
    got = buf.cpu().numpy().tobytes()
    assert got[:h.bytes] == pk.encode(img, *fr, sequence=9) and got[h.bytes:] == bytes([0x5a]) * CANARY
    r.close()


# ---- slots ----------------------------------------------------------------------------------------------------------------------------
def test_raw_and_coded_submits_alternate_over_the_slots():
    size, gaze, radii, uniform = SHAPES[0]
    r = _cornell(size, gaze, radii, uniform)
    views = [((size[0] // 2 + 17 * k) % size[0], (size[1] // 3 + 11 * k) % size[1]) for k in range(6)]
    codecs = [None, (1, 1, 0), None, (1, 1, 1), True, (0, 1, 0)]

    def setup(k):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = views[k]
        r.launchParams.frame.subframe_index = k

    def reference(frame, fr, k):
        if codecs[k] is None:
            return pk.encode(frame, *fr, sequence=500 + k)
        return bc.encode(frame, *fr, None if codecs[k] is True else codecs[k], sequence=500 + k)

    want = []
    for k in range(6):
        setup(k)
        r.render()
        want.append(reference(r.downloadPixels(), frame_of(r), k))
    slots, got = [], {}
    for k in range(6):
        setup(k)
        r.render_async()
        assert bytes(r.describePacket(500 + k, codecs[k])) == want[k][:128]
        slots.append(r.submitPacket(500 + k, codec=codecs[k]))
        if k >= 2:
            got[k - 2] = r.waitPacket(slots[k - 2])
    assert slots == [0, 1, 2, 3, 0, 1]
    for k in (4, 5):
        got[k] = r.waitPacket(slots[k])
    for k in range(6):
        assert got[k][:4] == (b"FVPK" if codecs[k] is None else b"FVPC") and got[k] == want[k], k
    assert len(want[1]) < len(want[5]) < len(want[0])
    assert r.waitPacket(2) == want[2] and r.waitPacket(3) == want[3]
    r.close()


# ---- error codes ----------------------------------------------------------------------------------------------------------------------
def test_error_codes_all_or_nothing():
    L = lib.load()
    size, gaze, radii, uniform = SHAPES[0]
    r = _cornell(size, gaze, radii, uniform)
    lp = C.byref(r.launchParams)
    hdr, slot = abi.PacketHeader(), C.c_int(-7)
    buf = device_filled(4096)
    good = abi.PacketConfig((1, 1, 0), 0)
    cfg = C.byref(good)

    def all_three(c):
        return (L.fovpt_packet_describe_coded(r._ctx, lp, c, 0, C.byref(hdr)), L.fovpt_packet_encode_coded(r._ctx, lp, c, None, 0, buf.data_ptr()),
                L.fovpt_packet_submit_coded(r._ctx, lp, c, None, 0, C.byref(slot)))

    def untouched():
        r.synchronize()
        return (buf.cpu().numpy() == 0x5a).all() and slot.value == -7

    assert all_three(cfg) == (E_NO_FRAME,) * 3                            # nothing rendered yet
    r.render()
    assert all_three(None) == (E_INVALID,) * 3 and b"null" in L.fovpt_last_error(r._ctx)
    assert L.fovpt_packet_describe_coded(None, lp, cfg, 0, C.byref(hdr)) == E_INVALID and L.fovpt_packet_describe_coded(r._ctx, None, cfg, 0, C.byref(hdr)) == E_INVALID
    assert L.fovpt_packet_describe_coded(r._ctx, lp, cfg, 0, None) == E_INVALID
    assert L.fovpt_packet_encode_coded(None, lp, cfg, None, 0, buf.data_ptr()) == E_INVALID and L.fovpt_packet_encode_coded(r._ctx, None, cfg, None, 0, buf.data_ptr()) == E_INVALID
    assert L.fovpt_packet_encode_coded(r._ctx, lp, cfg, None, 0, None) == E_INVALID
    assert L.fovpt_packet_encode_coded(r._ctx, lp, cfg, None, 0, buf.data_ptr() + 2) == E_INVALID      # not 4-byte aligned
    assert L.fovpt_packet_submit_coded(None, lp, cfg, None, 0, C.byref(slot)) == E_INVALID and L.fovpt_packet_submit_coded(r._ctx, None, cfg, None, 0, C.byref(slot)) == E_INVALID
    assert L.fovpt_packet_submit_coded(r._ctx, lp, cfg, None, 0, None) == E_INVALID
    for bad in (abi.PacketConfig((2, 0, 0), 0), abi.PacketConfig((0, 0, 0xfffffffe), 0), abi.PacketConfig((1, 256, 0), 0), abi.PacketConfig((1, 1, 0), 1)):
        assert all_three(C.byref(bad)) == (E_INVALID,) * 3
    f = r.launchParams.frame
    f.size.x -= 4
    assert all_three(cfg) == (E_NO_FRAME,) * 3                            # another frame size
    f.size.x += 4
    keep = f.frame_buffer
    f.frame_buffer = None
    assert all_three(cfg)[1:] == (E_NO_FRAME,) * 2                        # a null frame buffer
    f.frame_buffer = keep
    c = r.config
    c.world, c.rank = 2, 0
    r.config = c
    r.render()
    assert all_three(cfg) == (E_INVALID,) * 3 and b"world" in L.fovpt_last_error(r._ctx)      # a tile shard does not see the frame
    c.world, c.rank = 1, 0
    c.uniform = 1
    r.config = c
    r.render()
    assert all_three(cfg) == (E_INVALID,) * 3                             # FOV_OFF has one pass: codec[1] must be 0
    assert L.fovpt_packet_describe_coded(r._ctx, lp, C.byref(abi.PacketConfig((1, 0, 0), 0)), 0, C.byref(hdr)) == 0 and hdr.npass == 1
    c.uniform = 0
    r.config = c
    r.render()
    assert untouched()
    # the decoder refuses every header fovpt_packet_check refuses
    r.encodePacket(buf.data_ptr(), 3, None, (1, 1, 1))
    r.synchronize()
    packet = buf.cpu().numpy().tobytes()[:r.describePacket(3, (1, 1, 1)).bytes]
    assert packet == bc.encode(r.downloadPixels(), *frame_of(r), (1, 1, 1), sequence=3)
    out = upload(junk_canvas(size))
    refused = 0
    for label, m in coded_mutations(packet):
        if label.startswith(("another", "bytes above")) or len(m) != len(packet):      # (valid headers, or no header field changed)
            continue
        bad = abi.PacketHeader.from_packet(m)
        assert L.fovpt_packet_decode(r._ctx, C.byref(bad), buf.data_ptr(), 0, out.data_ptr()) == E_INVALID, label
        refused += 1
    assert refused >= 30
    r.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == JUNK).all()
    assert r.submitPacket(9, codec=(1, 1, 0)) == 0 and r.submitPacket(10) == 1      # none of the refused submits took a slot
    r.close()


# ---- a seeded sweep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("FOVPT_FUZZP_TO", "8"))))
def test_seeded_sweep(seed):
    rng = np.random.default_rng(5000 + seed)
    w, h = int(rng.integers(4, 97)), int(rng.integers(4, 81))      # (a side below 4 has no periphery launch index: no packet)
    uniform = bool(rng.random() < 0.2)
    ri = int(rng.integers(0, 12))
    radii = (ri, ri + int(rng.integers(0, 24)))
    gaze = (int(rng.integers(-8, w + 8)) & 0xffffffff, int(rng.integers(-8, h + 8)) & 0xffffffff)
    r = _cornell((w, h), gaze, radii, uniform, (1, 1, 1))
    r.render()
    frame = r.downloadPixels()
    fr = frame_of(r)
    npass = len(pk.passes(*fr))
    written = pk.owners(*fr)[0] >= 0
    mask = tuple(int(k) for k in rng.integers(0, 2, npass))
    if seed % 2 == 0:
        mask = (1,) * npass
    packet, dev = encode_on_device(r, seed, mask)
    assert packet == bc.encode(frame, *fr, mask, sequence=seed), (seed, fr, mask)
    hd = abi.PacketHeader.from_packet(packet)
    got = decode_on_device(r, dev, hd, abi.PACKET_NEAREST)
    assert np.array_equal(got != JUNK, written), (seed, fr, mask)
    img = random_frame((w, h), seed)
    keep = upload(img)
    packet, dev = encode_on_device(r, seed + 1, mask, keep.data_ptr())
    assert packet == bc.encode(img, *fr, mask, sequence=seed + 1), (seed, fr, mask)
    assert r.waitPacket(r.submitPacket(seed + 1, keep.data_ptr(), mask)) == packet
    for mode in (abi.PACKET_NEAREST, abi.PACKET_SMOOTH):
        want = bc.decode(packet, mode, junk_canvas((w, h)))
        assert np.array_equal(decode_on_device(r, dev, hd, mode), want), (seed, fr, mask, mode)
        assert np.array_equal(renderer.decode_packet(packet, mode, (w, h), out=junk_canvas((w, h))), want), (seed, fr, mask, mode)
    r.close()
