"""Foveated frame packets at BASELINE C3 (262,144-triangle atrium, 1920 x 1080, radii 148 / 482, spp 1 / 2 / 8) with two frames
in flight.  In one process, alternately, --reps times each, --frames frames after a warm-up, by the host clock around a loop
that ends in a device synchronise:
    DOWNLOAD  (a) render + downloadPixels per frame: today's way to see a frame (drains the pipeline, 8.3 MB to pageable memory)
    PACKET    (b) render + fovpt_packet_submit per frame, waiting for the slot submitted two frames earlier
    RENDER    (c) render alone: what nobody looking at a frame pays
and by HIP events on the library's stream around --calls calls back to back:
    ENCODE    (d) k_packet_encode alone (fovpt_packet_encode of the frame buffer)
    NEAREST / SMOOTH  k_packet_decode alone
Prints one JSON line: the median over the repetitions and the spread (min, max) of each, PACKET - RENDER beside RENDER's spread,
the bytes that cross to the host per frame, and the RMSE (8-bit codes, r g b) of decode(encode(x)) against x per foveation level
for x = fovpt_post's rgba8 output.  Kernel statistics are a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/packet_perf.py --frames 20 --calls 20 --reps 1
--coded measures coded packets ("FVPC") instead: the legs RENDER, PACKET, and render +
fovpt_packet_submit_coded with P and M as BC1 (CODED_110) and with all three levels as BC1 (CODED_111); k_packet_encode_coded and
the CODED decoders beside the raw kernels; the bytes per frame; and the RMSE per level of the decoded coded packet against
fovpt_post's output and against the decoded raw packet.
--depth measures depth packets ("FVPD") and the client's warp: the legs RENDER, PACKET (a colour submit per
frame) and a colour and a depth submit per frame with the call's own G-buffer trace (PACKET_DEPTH_TRACE) and with a caller's
G-buffer (PACKET_DEPTH_G); k_packet_depth_encode with a caller's G-buffer and with its own trace beside k_packet_encode;
k_packet_depth_decode beside NEAREST; fovpt_warp_depth beside fovpt_warp with a caller's G-buffer (a slide); the bytes; and for a
slide, a turn and a dolly-in the share of destination pixels whose source differs from the server's fovpt_warp, with both calls'
classes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fovpathtracing_optixcodelatest_amd import abi, renderer, scenes  # noqa: E402


def level_map(packet, size):
    """The fill of the texel each pixel decodes from (0: none), from the packet alone: its texels replaced by their pass's fill."""
    h = abi.PacketHeader.from_packet(packet)
    b = bytearray(packet)
    for p in range(h.npass):
        P = h.passes[p]
        tex = np.frombuffer(packet, "<u4", P.gw * P.gh, P.texels)
        b[P.texels:P.texels + 4 * P.gw * P.gh] = np.where(tex >> 24, 0xff000000 | P.fill, 0).astype("<u4").tobytes()
    return renderer.decode_packet(bytes(b), abi.PACKET_NEAREST, size) & 0xff


def scene(size):
    cfg = abi.Config.reference_default()
    cfg.r_inner, cfg.r_outer = 148, 482
    cfg.spp_periphery, cfg.spp_middle, cfg.spp_fovea = 1, 2, 8
    cfg.write_guides = 1
    cfg.frames_in_flight = 2
    r = renderer.SampleRenderer(scenes.atrium(262144))
    r.resize(size)
    cam = scenes.ATRIUM_CAMERA
    r.setCamera(renderer.Camera(cam["eye"], cam["lookat"], cam["up"], cam["fovy"], size[0] / size[1]))
    r.setProbe(renderer.ProbeData(scenes.ambient_probe(size[0], size[1], 2.5)).BuildCDF())
    r.config = cfg
    r.launchParams.frame.c.x, r.launchParams.frame.c.y = size[0] // 2, size[1] // 2
    r.render()
    return r


def timers(r, frames, warmup, calls):
    """per_frame(fn): ms per frame of fn(n) by the host clock; per_call(fn): ms per call by HIP events on the library's stream."""
    def per_frame(fn):
        fn(warmup)
        r.synchronize()
        t0 = time.perf_counter()
        fn(frames)
        r.synchronize()
        return (time.perf_counter() - t0) * 1e3 / frames

    st = torch.cuda.ExternalStream(r.stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def per_call(fn):
        for _ in range(max(1, warmup // 4)):
            fn()
        r.synchronize()
        a.record(st)
        for _ in range(calls):
            fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b) / calls

    return per_frame, per_call


def rgb(v):
    return np.stack([(v >> (8 * k)) & 0xff for k in range(3)], axis=-1).astype(np.float64)


def main_coded(frames, warmup, calls, reps):
    size = (1920, 1080)
    r = scene(size)
    per_frame, per_call = timers(r, frames, warmup, calls)
    codecs = {"PACKET": None, "CODED_110": (1, 1, 0), "CODED_111": (1, 1, 1)}
    headers = {k: r.describePacket(0, c) for k, c in codecs.items()}

    def leg_packet(codec):
        def run(n):
            slots = []
            for k in range(n):
                r.render_async()
                slots.append(r.submitPacket(k, codec=codec))
                if k >= 2:
                    r.waitPacket(slots[k - 2])
            for s in slots[-2:]:
                r.waitPacket(s)
        return run

    def leg_render(n):
        for _ in range(n):
            r.render_async()

    legs = dict(RENDER=leg_render)
    legs.update({k: leg_packet(c) for k, c in codecs.items()})
    dev = {k: torch.empty(h.bytes, dtype=torch.uint8, device="cuda") for k, h in headers.items()}
    out = torch.zeros((size[1], size[0]), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kernels = {}
    for k, c in codecs.items():
        kernels["ENCODE_" + k] = lambda k=k, c=c: r.encodePacket(dev[k].data_ptr(), 0, None, c)
    for k in codecs:                                              # (every buffer holds its packet by the time a decoder runs)
        for name, mode in (("NEAREST", abi.PACKET_NEAREST), ("SMOOTH", abi.PACKET_SMOOTH)):
            kernels["%s_%s" % (name, k)] = lambda k=k, mode=mode: r.decodePacket(headers[k], dev[k].data_ptr(), out.data_ptr(), mode)
    ms = {k: [] for k in list(legs) + list(kernels)}
    for _ in range(reps):                                         # alternately
        for k, fn in legs.items():
            ms[k].append(per_frame(fn))
        for k, fn in kernels.items():
            ms[k].append(per_call(fn))
    res = dict(config="C3", coded=True, size=list(size), frames_in_flight=2, frames=frames, calls=calls, reps=reps, device=torch.cuda.get_device_name(0))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k, v in ms.items():
        res["ms_" + k] = round(med[k], 4)
        res["spread_" + k] = [round(min(v), 4), round(max(v), 4)]
    for k in codecs:
        res[k + "_minus_RENDER"] = round(med[k] - med["RENDER"], 4)
        res["bytes_" + k] = int(headers[k].bytes)
    res["bytes_frame"] = size[0] * size[1] * 4

    # quality: the decoded coded packet of x = fovpt_post's rgba8 output against x and against the decoded raw packet, per level
    r.post()
    x = r.downloadPostPixels()
    decoded, rmse = {}, {}
    level = None
    for k, c in codecs.items():
        r.encodePacket(dev[k].data_ptr(), 0, r.post_buffers()[1], c)
        r.synchronize()
        packet = dev[k].cpu().numpy().tobytes()
        if c is None:
            level = level_map(packet, size)
        for name, mode in (("NEAREST", abi.PACKET_NEAREST), ("SMOOTH", abi.PACKET_SMOOTH)):
            out.zero_()
            torch.cuda.synchronize()
            r.decodePacket(headers[k], dev[k].data_ptr(), out.data_ptr(), mode)
            r.synchronize()
            y = out.cpu().numpy().view(np.uint32).copy()
            assert np.array_equal(y, renderer.decode_packet(packet, mode, size)), "device and host decoders differ"
            assert np.array_equal(y != 0, level > 0), "the coded packet writes another pixel set"
            decoded[k, name] = y
            for against, z in (("post", x), ("raw_packet", decoded["PACKET", name])):
                d2 = ((rgb(y) - rgb(z)) ** 2).mean(axis=-1)
                e = {("fill%d" % f): round(float(np.sqrt(d2[level == f].mean())), 3) for f in (1, 2, 4) if (level == f).any()}
                e["frame"] = round(float(np.sqrt(d2[level > 0].mean())), 3)
                rmse["%s_%s_vs_%s" % (k, name, against)] = e
    res["rmse"] = rmse
    res["pixels_per_level"] = {("fill%d" % f): int((level == f).sum()) for f in (0, 1, 2, 4)}
    print(json.dumps(res), flush=True)
    r.close()


def main_depth(frames, warmup, calls, reps):
    size = (1920, 1080)
    n = size[0] * size[1]
    r = scene(size)
    per_frame, per_call = timers(r, frames, warmup, calls)
    g = r.gbuffer()                                              # the rendered frame's: the camera does not move below
    r.synchronize()
    hc, hd = r.describePacket(), r.describeDepthPacket()

    def leg_render(k_frames):
        for _ in range(k_frames):
            r.render_async()

    def leg_submits(depth, gbuffer):
        def run(k_frames):
            slots = []
            for k in range(k_frames):
                r.render_async()
                mine = [r.submitPacket(k)]
                if depth:
                    mine.append(r.submitDepthPacket(k, gbuffer))
                slots.append(mine)
                if k >= 1:                                        # (four slots: a frame's two packets are waited for one frame later)
                    for s in slots[k - 1]:
                        r.waitPacket(s)
            for s in slots[-1]:
                r.waitPacket(s)
        return run

    legs = dict(RENDER=leg_render, PACKET=leg_submits(False, None), PACKET_DEPTH_TRACE=leg_submits(True, None), PACKET_DEPTH_G=leg_submits(True, g))
    dc = torch.empty(hc.bytes, dtype=torch.uint8, device="cuda")
    dd = torch.empty(hd.base.bytes, dtype=torch.uint8, device="cuda")
    rgba = torch.zeros((size[1], size[0]), dtype=torch.int32, device="cuda")
    depth = torch.zeros((size[1], size[0]), dtype=torch.float32, device="cuda")
    outs = [torch.zeros((size[1], size[0], c), dtype=torch.int32, device="cuda") for c in (4, 1, 1)]
    torch.cuda.synchronize()
    r.encodePacket(dc.data_ptr())
    r.encodeDepthPacket(dd.data_ptr(), 0, g)
    r.decodePacket(hc, dc.data_ptr(), rgba.data_ptr(), abi.PACKET_NEAREST)
    r.decodeDepthPacket(hd, dd.data_ptr(), depth.data_ptr())
    r.synchronize()
    cam = scenes.ATRIUM_CAMERA
    (ex, ey, ez), (lx, ly, lz) = cam["eye"], cam["lookat"]
    motions = dict(slide=((ex, ey, ez + 20.0), (lx, ly, lz + 20.0)), turn=((ex, ey, ez), (lx, ly, lz + 150.0)), dolly_in=((ex + 100.0, ey, ez), (lx, ly, lz)))
    tos = {k: r.warp_camera(renderer.Camera(e, l, cam["up"], cam["fovy"], size[0] / size[1])) for k, (e, l) in motions.items()}
    accum, frame = r.launchParams.frame.accum_buffer, r.launchParams.frame.frame_buffer
    kernels = dict(ENCODE=lambda: r.encodePacket(dc.data_ptr()),
                   ENCODE_DEPTH_G=lambda: r.encodeDepthPacket(dd.data_ptr(), 0, g),
                   ENCODE_DEPTH_TRACE=lambda: r.encodeDepthPacket(dd.data_ptr(), 0),
                   NEAREST=lambda: r.decodePacket(hc, dc.data_ptr(), rgba.data_ptr(), abi.PACKET_NEAREST),
                   DECODE_DEPTH=lambda: r.decodeDepthPacket(hd, dd.data_ptr(), depth.data_ptr()),
                   WARP_G=lambda: r.warp(tos["slide"], None, g, None, None, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr()),
                   WARP_DEPTH=lambda: r.warp_depth(size, depth.data_ptr(), hd.camera, tos["slide"], None, accum, frame, outs[0].data_ptr(),
                                                   outs[1].data_ptr(), outs[2].data_ptr()))
    ms = {k: [] for k in list(legs) + list(kernels)}
    for _ in range(reps):                                         # alternately
        for k, fn in legs.items():
            ms[k].append(per_frame(fn))
        for k, fn in kernels.items():
            ms[k].append(per_call(fn))
    res = dict(config="C3", depth=True, size=list(size), frames_in_flight=2, frames=frames, calls=calls, reps=reps, device=torch.cuda.get_device_name(0))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k, v in ms.items():
        res["ms_" + k] = round(med[k], 4)
        res["spread_" + k] = [round(min(v), 4), round(max(v), 4)]
    for k in ("PACKET", "PACKET_DEPTH_TRACE", "PACKET_DEPTH_G"):
        res[k + "_minus_RENDER"] = round(med[k] - med["RENDER"], 4)
    res["bytes_colour"], res["bytes_depth"], res["bytes_frame"] = int(hc.bytes), int(hd.base.bytes), n * 4

    # what the client's warp shows against the server's: per motion the share of destination pixels whose source differs, and the classes
    r.render()
    r.encodeDepthPacket(dd.data_ptr(), 0)
    r.decodeDepthPacket(hd, dd.data_ptr(), depth.data_ptr())
    g = r.gbuffer()
    agree = {}
    for name, to in tos.items():
        maps, shares = [], []
        for client in (False, True):
            if client:
                r.warp_depth(size, depth.data_ptr(), hd.camera, to, None, accum, frame, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
            else:
                r.warp(to, None, g, None, None, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
            c = r.warp_counts()
            shares.append(dict(direct=round(c.direct / n, 4), filled=round(c.filled / n, 4), empty=round(c.empty / n, 4)))
            maps.append(outs[2].cpu().numpy().view(np.uint32).reshape(-1).copy())
        agree[name] = dict(source_differs=round(float(((maps[0] & 0x3fffffff) != (maps[1] & 0x3fffffff)).mean()), 4), server=shares[0], client=shares[1])
    res["warp"] = agree
    print(json.dumps(res), flush=True)
    r.close()


def main(frames, warmup, calls, reps):
    size = (1920, 1080)
    r = scene(size)
    header = r.describePacket()

    def leg_download(n):
        for _ in range(n):
            r.render_async()
            r.downloadPixels()

    def leg_packet(n):
        slots = []
        for k in range(n):
            r.render_async()
            slots.append(r.submitPacket(k))
            if k >= 2:
                r.waitPacket(slots[k - 2])
        for s in slots[-2:]:
            r.waitPacket(s)

    def leg_render(n):
        for _ in range(n):
            r.render_async()

    legs = dict(DOWNLOAD=leg_download, PACKET=leg_packet, RENDER=leg_render)

    per_frame, per_call = timers(r, frames, warmup, calls)
    # (d) the kernels alone
    dev = torch.empty(header.bytes, dtype=torch.uint8, device="cuda")
    out = torch.zeros((size[1], size[0]), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kernels = dict(ENCODE=lambda: r.encodePacket(dev.data_ptr()),
                   NEAREST=lambda: r.decodePacket(header, dev.data_ptr(), out.data_ptr(), abi.PACKET_NEAREST),
                   SMOOTH=lambda: r.decodePacket(header, dev.data_ptr(), out.data_ptr(), abi.PACKET_SMOOTH))
    ms = {k: [] for k in list(legs) + list(kernels)}
    for _ in range(reps):                                     # alternately
        for k, fn in legs.items():
            ms[k].append(per_frame(fn))
        for k, fn in kernels.items():
            ms[k].append(per_call(fn))
    res = dict(config="C3", size=list(size), frames_in_flight=2, frames=frames, calls=calls, reps=reps, device=torch.cuda.get_device_name(0))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k, v in ms.items():
        res["ms_" + k] = round(med[k], 4)
        res["spread_" + k] = [round(min(v), 4), round(max(v), 4)]
    res["PACKET_minus_RENDER"] = round(med["PACKET"] - med["RENDER"], 4)
    res["DOWNLOAD_minus_RENDER"] = round(med["DOWNLOAD"] - med["RENDER"], 4)
    res["PACKET_below_DOWNLOAD"] = bool(max(ms["PACKET"]) < min(ms["DOWNLOAD"]))
    res["bytes_packet"], res["bytes_frame"] = int(header.bytes), size[0] * size[1] * 4
    res["bytes_ratio"] = round(res["bytes_frame"] / res["bytes_packet"], 2)

    # what the packet costs in quality: decode(encode(x)) against x = fovpt_post's rgba8 output, per level
    r.post()
    x = r.downloadPostPixels()
    r.encodePacket(dev.data_ptr(), 0, r.post_buffers()[1])
    r.synchronize()
    packet = dev.cpu().numpy().tobytes()
    level = level_map(packet, size)
    rmse = {}
    for name, mode in (("NEAREST", abi.PACKET_NEAREST), ("SMOOTH", abi.PACKET_SMOOTH)):
        out.zero_()
        torch.cuda.synchronize()
        r.decodePacket(header, dev.data_ptr(), out.data_ptr(), mode)
        r.synchronize()
        y = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(y, renderer.decode_packet(packet, mode, size)), "device and host decoders differ"
        d2 = ((rgb(y) - rgb(x)) ** 2).mean(axis=-1)
        rmse[name] = {("fill%d" % f): round(float(np.sqrt(d2[level == f].mean())), 3) for f in (1, 2, 4) if (level == f).any()}
        rmse[name]["frame"] = round(float(np.sqrt(d2[level > 0].mean())), 3)
    res["rmse"] = rmse
    res["pixels_per_level"] = {("fill%d" % f): int((level == f).sum()) for f in (0, 1, 2, 4)}
    print(json.dumps(res), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--coded", action="store_true", help="coded packets (BC1 levels) beside raw ones")
    ap.add_argument("--depth", action="store_true", help="depth packets and the client's warp beside the colour packet and fovpt_warp")
    args = ap.parse_args()
    (main_depth if args.depth else main_coded if args.coded else main)(args.frames, args.warmup, args.calls, args.reps)
