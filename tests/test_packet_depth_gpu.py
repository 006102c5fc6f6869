"""Depth packets and fovpt_warp_depth on the GPU against tests/packet_depth_ref.py and tests/warp_depth_ref.py, bit for bit: the
encoder on traced and on uploaded G-buffers, the device decoder against the restatement and the host decoder, the warp for three
camera motions on decoded and on synthetic depth images, the identity, the rejections, a client context that holds no scene, the
slots shared with the colour packets, a seeded sweep and the C++ drop-in.  The scene is the box scene of tests/gpu_common.py (it
has sky around it) at the shapes of tests/packet_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import packet_depth_ref as pd
import packet_ref as pk
import warp_depth_ref as wd
import warp_ref as wr
from fovpathtracing_optixcodelatest_amd import abi, abi_depth, lib, renderer

from common import cfg_foveated, cfg_uniform
from gpu_common import bits, box_renderer, build_dropin, camera, device_filled, device_images, host_view, run_dropin, upload, with_entries
from packet_cases import IDS, JUNK, SHAPES, junk_canvas, random_frame
from packet_depth_cases import JUNK_DEPTH, camera_dict, junk_depth, mutations, synthetic_depth, synthetic_gbuffer

pytestmark = pytest.mark.gpu
E_INVALID, E_NO_SCENE, E_NO_FRAME = -1, -3, -5
# eye, lookat of the camera to warp to: the motions of tests/test_warp_gpu.py
MOTIONS = dict(identity=((4.0, 3.0, 6.0), (0.0, 0.5, 0.0)), slide=((4.333, 3.0, 5.778), (0.333, 0.5, -0.222)),
               turn=((4.0, 3.0, 6.0), (1.2, 0.5, -1.0)), dolly_in=((3.2, 2.5, 4.8), (0.0, 0.5, 0.0)))


def box(shape, spp=(1, 1, 2)):
    size, gaze, radii, uniform = shape
    return box_renderer(size, cfg_uniform(1) if uniform else cfg_foveated(radii[0], radii[1], spp), gaze=gaze)


def to_camera(motion, size):
    return camera_dict(size, *MOTIONS[motion])


def wcfg(**d):
    return with_entries(renderer.SampleRenderer.warp_defaults(), d)


def gbuffer_ptrs(size, prim, position):
    g = abi.GBufferPtrs()
    g.prim, g.position, g.width, g.height = prim.data_ptr(), position.data_ptr(), size[0], size[1]
    return g


def encode_on_device(r, sequence, gbuffer=None, near=None):
    """fovpt_packet_encode_depth into a junk-filled buffer 64 bytes longer than the packet -> (the packet's bytes, the buffer,
    the header); the tail stays junk."""
    h = r.describeDepthPacket(sequence, near)
    buf = device_filled(h.base.bytes + 64)
    h2 = r.encodeDepthPacket(buf.data_ptr(), sequence, gbuffer, near)
    assert bytes(h) == bytes(h2)
    r.synchronize()
    got = buf.cpu().numpy().tobytes()
    assert got[h.base.bytes:] == bytes([0x5a]) * 64
    assert got[:192] == bytes(h)
    return got[:h.base.bytes], buf, h


def decode_on_device(r, packet_dev, header):
    out = upload(junk_depth((header.base.width, header.base.height)))
    r.decodeDepthPacket(header, packet_dev.data_ptr(), out.data_ptr())
    r.synchronize()
    return out.cpu().numpy()


def warp_on_device(r, size, depth, frm, to, radius=2, images=3, seed=0):
    """One fovpt_warp_depth of random images against the restatement: every pixel of every enabled output, the map, the counts;
    an image that is not enabled keeps its bytes.  -> the restatement's output."""
    w, h = size
    rng = np.random.default_rng(seed)
    color = rng.uniform(0, 8, (h, w, 4)).astype(np.float32)
    color.reshape(-1, 4)[rng.permutation(w * h)[:16]] = (np.nan, np.inf, -0.0, 1e-42)      # copied bit for bit, whatever they hold
    rgba = random_frame(size, seed + 1)
    dev = [upload(a) for a in (np.ascontiguousarray(depth, np.float32), color, rgba)]
    oc, op, om = device_images(size, 16, 4, 4)
    r.warp_depth(size, dev[0].data_ptr(), frm, to, wcfg(images=images, fill_radius=radius), dev[1].data_ptr(), dev[2].data_ptr(),
                 oc.data_ptr(), op.data_ptr(), om.data_ptr())
    n = r.warp_counts()
    got_counts = (n.splatted, n.direct, n.filled, n.empty)
    want = wd.warp(depth, frm, to, dict(images=images, fill_radius=radius), color, rgba)
    assert np.array_equal(host_view(om, "map"), want["map"])
    assert got_counts == want["counts"] and sum(got_counts[1:]) == w * h, (got_counts, want["counts"])
    if images & wr.COLOR:
        assert np.array_equal(bits(host_view(oc, "color")), bits(want["color"]))
    else:
        assert (oc.cpu().numpy() == 0x5a).all()
    if images & wr.RGBA:
        assert np.array_equal(host_view(op, "rgba"), want["rgba"])
    else:
        assert (op.cpu().numpy() == 0x5a).all()
    assert np.array_equal(dev[0].cpu().numpy().view(np.uint32), bits(depth))      # the depth image is as it was
    return want


# ---- 1. encode, decode and warp at the six shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_encode_decode_and_warp_bit_for_bit(k):
    size, gaze, radii, uniform = SHAPES[k]
    r = box(SHAPES[k])
    r.render()
    gb, cam = r.downloadGBuffer(), camera(r)
    assert (gb["prim"] == wr.MISS).any() and (gb["prim"] != wr.MISS).any()             # sky and surfaces
    want = pd.encode(gb, cam, pd.DEFAULT_NEAR, size, gaze, radii, uniform, sequence=11)
    got, buf, header = encode_on_device(r, 11)                                        # the call's own trace
    assert got == want, sum(a != b for a, b in zip(got, want))
    assert encode_on_device(r, 11, r.gbuffer())[0] == want                            # fovpt_gbuffer's pointers
    assert encode_on_device(r, 11, None, 0.05)[0] == pd.encode(gb, cam, 0.05, size, gaze, radii, uniform, sequence=11)
    # an uploaded synthetic G-buffer: every kind of code, texels that own sky and hit pixels
    syn = synthetic_gbuffer(size, cam, 60 + k)
    sp, sx = upload(syn["prim"]), upload(syn["position"])
    want_syn = pd.encode(syn, cam, pd.DEFAULT_NEAR, size, gaze, radii, uniform, sequence=12)
    got_syn, buf_syn, header_syn = encode_on_device(r, 12, gbuffer_ptrs(size, sp, sx))
    assert got_syn == want_syn, sum(a != b for a, b in zip(got_syn, want_syn))
    assert {1, 2, 65535} <= set(np.unique(pd.pixel_codes(syn, cam, pd.DEFAULT_NEAR)).tolist())
    # the device decoder against the restatement and the host decoder, on a junk canvas
    for packet, dev, hd in ((got, buf, header), (got_syn, buf_syn, header_syn)):
        depth = decode_on_device(r, dev, hd)
        ref = pd.decode(packet, junk_depth(size))
        assert np.array_equal(bits(depth), bits(ref))
        assert np.array_equal(bits(renderer.decode_depth_packet(packet, size, out=junk_depth(size))), bits(ref))
        written = pk.owners(size, gaze, radii, uniform)[0] >= 0
        assert (depth[~written] == JUNK_DEPTH).all() and (depth[written] > 0).all()
    # the warp from the decoded depths (the junk of unwritten pixels is negative: they scatter nothing), three motions
    depth = decode_on_device(r, buf, header)
    assert np.isinf(depth).any() and np.isfinite(depth[depth > 0]).any()
    collide = 0
    for j, motion in enumerate(("slide", "turn", "dolly_in")):
        o = warp_on_device(r, size, depth, cam, to_camera(motion, size), radius=(2, 0, 4)[j], images=(3, 2, 1)[j], seed=10 * k + j)
        assert o["counts"][1] > size[0] * size[1] // 8, motion              # (the motions keep the scene in view)
        collide += int((wr.collisions(o["dest"]) >= 2).sum())
    assert collide > 0                                                    # the depth test had something to decide
    o = warp_on_device(r, size, synthetic_depth(size, 80 + k), cam, to_camera("slide", size), seed=k)
    assert o["counts"][3] > 0 or o["counts"][2] > 0
    # the identity: every pixel that scatters lands on itself, on the device
    o = warp_on_device(r, size, depth, cam, cam, radius=0, images=2, seed=k)
    live = depth > 0
    own = np.arange(size[0] * size[1]).reshape(size[1], size[0])
    assert np.array_equal(o["dest"][live], own[live]) and o["counts"][0] == int(live.sum())
    r.close()


# ---- 2. a client that holds no scene -----------------------------------------------------------------------------------------------------
def test_a_client_context_decodes_both_packets_and_warps():
    size, gaze, radii, uniform = SHAPES[4]
    server = box(SHAPES[4])
    server.render()
    sc, sd = server.submitPacket(1), server.submitDepthPacket(2)
    colour, deep = server.waitPacket(sc), server.waitPacket(sd)
    assert pk.check(colour) and pd.check(deep) and len(deep) < len(colour)
    assert deep == pd.encode(server.downloadGBuffer(), camera(server), pd.DEFAULT_NEAR, size, gaze, radii, uniform, sequence=2)
    L = lib.load()
    ctx = C.c_void_p()
    assert L.fovpt_create(C.byref(ctx), 0) == 0                          # no scene, no resize, no render
    try:
        hc, hd = abi.PacketHeader.from_packet(colour), abi_depth.PacketDepthHeader.from_packet(deep)
        dc, dd = upload(np.frombuffer(colour, np.uint8).copy()), upload(np.frombuffer(deep, np.uint8).copy())
        rgba, depth = upload(junk_canvas(size)), upload(junk_depth(size))
        assert L.fovpt_packet_decode(ctx, C.byref(hc), dc.data_ptr(), abi.PACKET_NEAREST, rgba.data_ptr()) == 0
        assert L.fovpt_packet_decode_depth(ctx, C.byref(hd), dd.data_ptr(), depth.data_ptr()) == 0, L.fovpt_last_error(ctx)
        to = renderer.SampleRenderer.warp_camera(to_camera("slide", size))
        op, om = device_images(size, 4, 4)
        cfg = wcfg(images=abi.WARP_RGBA)
        rc = L.fovpt_warp_depth(ctx, size[0], size[1], C.byref(hd.camera), C.byref(to), C.byref(cfg), depth.data_ptr(), None, rgba.data_ptr(), None,
                                op.data_ptr(), om.data_ptr())
        assert rc == 0, L.fovpt_last_error(ctx)
        counts = abi.WarpCounts()
        assert L.fovpt_warp_counts(ctx, C.byref(counts)) == 0
        # the restatements, from the two packets' bytes alone
        want_rgba = pk.decode(colour, pk.NEAREST, junk_canvas(size))
        want_depth = pd.decode(deep, junk_depth(size))
        frm = pd.parse(deep)["camera"]
        want = wd.warp(want_depth, frm, to_camera("slide", size), dict(images=wr.RGBA, fill_radius=2), None, want_rgba)
        assert np.array_equal(bits(depth.cpu().numpy()), bits(want_depth))
        assert np.array_equal(host_view(op, "rgba"), want["rgba"]) and np.array_equal(host_view(om, "map"), want["map"])
        assert (counts.splatted, counts.direct, counts.filled, counts.empty) == want["counts"] and want["counts"][1] > size[0] * size[1] // 2
        assert frm == camera(server)                                     # the header carries the rendered camera
        # what needs a frame still refuses this context
        lp = abi.LaunchParams()
        assert L.fovpt_packet_describe_depth(ctx, C.byref(lp), C.byref(server.depthPacketConfig()), 0, C.byref(hd)) == E_NO_FRAME
    finally:
        L.fovpt_destroy(ctx)
    server.close()


# ---- 3. the slots, shared with the colour packets ---------------------------------------------------------------------------------------
def test_colour_and_depth_submits_share_the_slots():
    size, _, radii, _ = SHAPES[0]
    r = box(SHAPES[0], (1, 1, 1))
    gazes = [(32, 24), (10, 40), (60, 5), (0, 0), (63, 47), (20, 12)]
    got = []
    for start in (0, 2, 4):                                               # two frames in the four slots at a time
        pending = []
        for k in (start, start + 1):
            r.launchParams.frame.c.x, r.launchParams.frame.c.y = gazes[k]
            r.launchParams.frame.subframe_index = k
            r.render_async()                                              # the next frame is rendered at once
            pending.append((k, r.submitPacket(100 + k), r.submitDepthPacket(200 + k)))
        for k, sc, sd in pending:
            assert (sc, sd) == ((2 * k) % 4, (2 * k + 1) % 4)
            got.append((r.waitPacket(sc), r.waitPacket(sd)))
    for k, g in enumerate(gazes):
        r.launchParams.frame.c.x, r.launchParams.frame.c.y = g
        r.launchParams.frame.subframe_index = k
        r.render()
        colour = pk.encode(r.downloadPixels(), size, g, radii, False, sequence=100 + k)
        deep = pd.encode(r.downloadGBuffer(), camera(r), pd.DEFAULT_NEAR, size, g, radii, False, sequence=200 + k)
        assert got[k][0] == colour and got[k][1] == deep, k
    assert len({p for p, _ in got}) == 6 and len({p for _, p in got}) > 1
    r.close()


# ---- 4. rejections --------------------------------------------------------------------------------------------------------------------
def test_rejections_all_or_nothing():
    size, gaze, radii, uniform = SHAPES[0]
    w, h = size
    r = box(SHAPES[0])
    L = lib.load()
    buf = device_filled(8192)
    with pytest.raises(lib.FovptError) as e:                              # nothing rendered yet
        r.encodeDepthPacket(buf.data_ptr())
    assert e.value.code == E_NO_FRAME
    r.render()
    g = r.gbuffer()
    packet, dev, header = encode_on_device(r, 1)
    cam = camera(r)
    before = None

    def refuse_encode(code, label, **kw):
        with pytest.raises(lib.FovptError) as e:
            r.encodeDepthPacket(buf.data_ptr(), **kw)
        assert e.value.code == code, label
        with pytest.raises(lib.FovptError) as e:
            r.submitDepthPacket(**kw)
        assert e.value.code == code, label
        assert (buf.cpu().numpy() == 0x5a).all(), label

    for near in (0.0, -0.1, float("nan"), float("inf")):
        refuse_encode(E_INVALID, ("near", near), near=near)
    c = r.depthPacketConfig()
    c._reserved[2] = 1
    refuse_encode(E_INVALID, "reserved", near=c)
    for k, v in (("width", w - 1), ("height", h + 1), ("prim", None), ("position", None)):
        bad = abi.GBufferPtrs.from_buffer_copy(bytes(g))
        setattr(bad, k, v)
        refuse_encode(E_INVALID, ("gbuffer", k), gbuffer=bad)
    with pytest.raises(lib.FovptError) as e:
        r.encodeDepthPacket(buf.data_ptr() + 2)
    assert e.value.code == E_INVALID
    lp, cfg = C.byref(r.launchParams), C.byref(r.depthPacketConfig())
    assert L.fovpt_packet_encode_depth(r._ctx, None, cfg, None, 0, buf.data_ptr()) == E_INVALID
    assert L.fovpt_packet_encode_depth(r._ctx, lp, None, None, 0, buf.data_ptr()) == E_INVALID
    assert L.fovpt_packet_encode_depth(r._ctx, lp, cfg, None, 0, None) == E_INVALID
    assert L.fovpt_packet_submit_depth(r._ctx, lp, cfg, None, 0, None) == E_INVALID
    assert L.fovpt_packet_describe_depth(r._ctx, lp, cfg, 0, None) == E_INVALID
    keep = r.launchParams.traversable
    r.launchParams.traversable = keep + 1                                 # not the current scene: only the traced G-buffer needs it
    refuse_encode(E_NO_SCENE, "no scene")
    assert encode_on_device(r, 1, g)[0] == packet
    r.launchParams.traversable = keep
    # the device decoder: every mutation of the header, and the colour decoder on a depth packet
    out = upload(junk_depth(size))
    for label, m in mutations(packet):
        if label.startswith("another") or label.startswith("bytes above"):   # (valid headers: of another output, of a longer buffer)
            continue
        hd = abi_depth.PacketDepthHeader.from_packet(m)
        assert L.fovpt_packet_decode_depth(r._ctx, C.byref(hd), dev.data_ptr(), out.data_ptr()) == E_INVALID, label
    r.synchronize()
    assert (out.cpu().numpy() == JUNK_DEPTH).all()
    assert L.fovpt_packet_decode(r._ctx, C.byref(header.base), dev.data_ptr(), 0, out.data_ptr()) == E_INVALID
    assert L.fovpt_packet_decode_depth(r._ctx, C.byref(header), dev.data_ptr() + 2, out.data_ptr()) == E_INVALID
    assert L.fovpt_packet_decode_depth(r._ctx, None, dev.data_ptr(), out.data_ptr()) == E_INVALID
    assert L.fovpt_packet_decode_depth(r._ctx, C.byref(header), None, out.data_ptr()) == E_INVALID
    assert L.fovpt_packet_decode_depth(r._ctx, C.byref(header), dev.data_ptr(), None) == E_INVALID
    far = abi_depth.PacketDepthHeader.from_packet(packet)
    far.base.passes[0].factor = 1 << 28                                   # a valid header the device decoder's search cannot take
    assert pd.check(bytes(far) + packet[192:]) and L.fovpt_packet_decode_depth(r._ctx, C.byref(far), dev.data_ptr(), out.data_ptr()) == E_INVALID
    # fovpt_warp_depth
    depth = upload(decode_on_device(r, dev, header))
    to = to_camera("slide", size)
    ic, ip = upload(np.zeros((h, w, 4), np.float32)), upload(random_frame(size, 3))
    oc, op, om = device_images(size, 16, 4, 4)
    r.warp_depth(size, depth.data_ptr(), cam, to, None, ic.data_ptr(), ip.data_ptr(), oc.data_ptr(), op.data_ptr(), om.data_ptr())
    r.synchronize()
    before = [t.cpu().numpy().tobytes() for t in (oc, op, om)] + [bytes(r.warp_counts())]
    good = dict(size=size, depth=depth.data_ptr(), from_camera=cam, to=to, cfg=None, in_color=ic.data_ptr(), in_rgba=ip.data_ptr(),
                out_color=oc.data_ptr(), out_rgba=op.data_ptr(), out_map=om.data_ptr())

    def refuse(label, **kw):
        with pytest.raises(lib.FovptError) as e:
            r.warp_depth(**dict(good, **kw))
        assert e.value.code == E_INVALID, label
        assert [t.cpu().numpy().tobytes() for t in (oc, op, om)] + [bytes(r.warp_counts())] == before, label

    for bad in ((0, h), (w, 0), (-1, h), (1 << 15, 1 << 15), (1 << 16, 1 << 14)):
        refuse(("size", bad), size=bad)
    for images in (0, 4, -1):
        refuse(("images", images), cfg=wcfg(images=images))
    for radius in (-1, abi.WARP_MAX_RADIUS + 1):
        refuse(("fill_radius", radius), cfg=wcfg(fill_radius=radius))
    c = wcfg()
    c._reserved[5] = 1
    refuse("reserved", cfg=c)
    for which in ("from_camera", "to"):
        for key in ("eye", "U", "V", "W"):
            for v in (float("nan"), float("inf")):
                refuse((which, key, v), **{which: dict(good[which], **{key: (good[which][key][0], v, good[which][key][2])})})
        refuse((which, "singular"), **{which: dict(good[which], W=good[which]["U"])})
    refuse("null depth", depth=None)
    refuse("null in_color", in_color=None)
    refuse("null out_rgba", out_rgba=None)
    refuse("null out_color", out_color=None)
    refuse("out_color is in_color", out_color=ic.data_ptr())
    refuse("out_rgba is the depth", out_rgba=depth.data_ptr())
    refuse("out_map is in_rgba", out_map=ip.data_ptr())
    refuse("out_map is out_rgba", out_map=op.data_ptr())
    refuse("out_rgba is out_color", out_rgba=oc.data_ptr())
    fr, tc = (renderer.SampleRenderer.warp_camera(x) for x in (cam, to))
    wc = wcfg()
    args = [depth.data_ptr(), ic.data_ptr(), ip.data_ptr(), oc.data_ptr(), op.data_ptr(), om.data_ptr()]
    assert L.fovpt_warp_depth(r._ctx, w, h, None, C.byref(tc), C.byref(wc), *args) == E_INVALID
    assert L.fovpt_warp_depth(r._ctx, w, h, C.byref(fr), None, C.byref(wc), *args) == E_INVALID
    assert L.fovpt_warp_depth(r._ctx, w, h, C.byref(fr), C.byref(tc), None, *args) == E_INVALID
    # an image that is not enabled needs no buffers; the valid call after them; fovpt_warp's keys are not this call's
    r.warp_depth(size, depth.data_ptr(), cam, to, wcfg(images=abi.WARP_RGBA), None, ip.data_ptr(), None, op.data_ptr(), None)
    r.warp(to)
    mine = r.warp_counts()
    r.warp_depth(**good)
    r.synchronize()
    assert [t.cpu().numpy().tobytes() for t in (oc, op, om)] + [bytes(r.warp_counts())] == before and bytes(mine) != before[3]
    r.close()


# ---- 5. a seeded sweep --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("FOVPT_FUZZD_TO", "8"))))
def test_seeded_sweep(seed):
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(8, 97)), int(rng.integers(8, 97))
    uniform = bool(rng.integers(0, 4) == 0)
    gaze = (int(rng.integers(0, w)), int(rng.integers(0, h)))
    r_inner = int(rng.integers(2, 12))
    radii = (r_inner, r_inner + int(rng.integers(2, 24)))
    near = float(np.float32(np.exp(rng.uniform(np.log(0.01), np.log(2.0)))))
    size = (w, h)
    r = box((size, gaze, radii, uniform), (1, 1, 1))
    r.render()
    gb, cam = r.downloadGBuffer(), camera(r)
    try:
        header = r.describeDepthPacket(seed, near)
    except lib.FovptError as e:                                           # a pass without a launch index: no packet, colour or depth
        assert e.code == E_INVALID
        with pytest.raises(lib.FovptError):
            r.describePacket(seed)
        r.close()
        return
    got, buf, header = encode_on_device(r, seed, None, near)
    assert got == pd.encode(gb, cam, near, size, gaze, None if uniform else radii, uniform, sequence=seed), (size, gaze, radii, uniform, near)
    depth = decode_on_device(r, buf, header)
    assert np.array_equal(bits(depth), bits(pd.decode(got, junk_depth(size))))
    eye = tuple(float(v) for v in np.asarray(MOTIONS["identity"][0]) + rng.uniform(-0.8, 0.8, 3))
    lookat = tuple(float(v) for v in np.asarray(MOTIONS["identity"][1]) + rng.uniform(-0.8, 0.8, 3))
    warp_on_device(r, size, depth, cam, camera_dict(size, eye, lookat), radius=int(rng.integers(0, 5)), images=int(rng.integers(1, 4)), seed=seed)
    r.close()


# ---- 6. the C++ drop-in -------------------------------------------------------------------------------------------------------------------
def test_cpp_dropin_depth_packets(tmp_path):
    """submitDepthPacket / decodeDepthPacket / warpDepth of include/SimplePathtracer.h: the program's packets, depths, warped
    pixels, map and counts are the restatements' of its own two packets."""
    exe = build_dropin(tmp_path, "packet_depth_gpu_test", extra=["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    out = str(tmp_path / "packet_depth_out.bin")
    run_dropin(exe, out)
    size = (160, 96)
    n = size[0] * size[1]
    raw = open(out, "rb").read()
    nc, nd = np.frombuffer(raw, np.uint32, 2)
    colour, deep = raw[8:8 + nc], raw[8 + nc:8 + nc + nd]
    at = 8 + int(nc) + int(nd)
    depth = np.frombuffer(raw, np.float32, n, at).reshape(size[1], size[0])
    warped = np.frombuffer(raw, np.uint32, n, at + 4 * n).reshape(size[1], size[0])
    wmap = np.frombuffer(raw, np.uint32, n, at + 8 * n).reshape(size[1], size[0])
    counts = tuple(int(v) for v in np.frombuffer(raw, np.uint64, 4, at + 12 * n))
    assert pk.check(colour) and pd.check(deep)
    hd = pd.parse(deep)
    assert np.array_equal(bits(depth), bits(pd.decode(deep, np.zeros((size[1], size[0]), np.float32))))
    rgba = pk.decode(colour, pk.NEAREST, np.zeros((size[1], size[0]), np.uint32))
    want = wd.warp(depth, hd["camera"], camera_dict(size, (3.5, 3.0, 6.5), (0.0, 0.5, 0.0)), dict(images=wr.RGBA, fill_radius=2), None, rgba)
    assert np.array_equal(warped, want["rgba"]) and np.array_equal(wmap, want["map"]) and counts == want["counts"]
    assert counts[1] > n // 2 and counts[2] > 0 and len(np.unique(warped)) > 20
