"""numpy restatement of the depth packet "FVPD" (include/fovpt.h, fovpt_packet_*_depth; csrc/packet.hip, k_packet_depth_*, and
csrc/packet_host.cpp): the definition the device encoder, the device decoder and the host decoder match bit for bit.  Built on
packet_ref's passes and owners: a depth packet's texels are those of the colour packet of the same frame.

    layout    192-byte header, then per pass gw * gh uint16 codes, row-major ly * gw + lx, and 0 or 2 zero bytes up to a multiple
              of 4, back to back; little endian
    header    words 0 .. 31: packet_ref's header with magic "FVPD", the pass offsets those of the code arrays; 32 .. 43: eye, U,
              V, W of the rendered camera; 44: near; 45 .. 47: 0
    code      of a pixel, every operation binary32, M the rows of inverse([U V W]) (temporal_ref.camera_inverse):
              prim == 0xffffffff -> 1; v = X - eye, z = (M_2.x v.x + M_2.y v.y) + M_2.z v.z; not (z > 0) or z not finite -> 1;
              q = near / z, c = floor(q * 65534 + 0.5) clamped to [1, 65534], code = c + 1
              of a texel: 0 where it owns no pixel, else the largest code of the pixels it owns
    decode    a pixel takes the last texel with code != 0 whose block reaches it (packet_ref's NEAREST write order): +inf for
              code 1, else (near * 65534) / (code - 1); other pixels keep what out held"""
import struct

import numpy as np

import packet_ref as pk
import temporal_ref as tr

f32 = np.float32
MAGIC, VERSION, HEADER_BYTES = 0x44505646, 1, 192
MISS = np.uint32(0xffffffff)
M32 = 0xffffffff
DEFAULT_NEAR = f32(0.1)


def pixel_codes(gb, cam, near):
    """gb: dict prim (h, w) uint32, position (h, w, 4) float32; cam: dict eye / U / V / W -> (h, w) int64 codes 1 .. 65535."""
    M = tr.camera_inverse(cam["U"], cam["V"], cam["W"])
    assert M is not None
    near = f32(near)
    X = np.ascontiguousarray(gb["position"][..., :3], np.float32)
    with np.errstate(all="ignore"):
        v = X - np.asarray(cam["eye"], np.float32)
        z = (M[2, 0] * v[..., 0] + M[2, 1] * v[..., 1]) + M[2, 2] * v[..., 2]
        assert z.dtype == np.float32
        q = near / z
        c = np.floor(q * f32(65534.0) + f32(0.5))
        c = np.maximum(f32(1.0), np.minimum(c, f32(65534.0)))
        assert c.dtype == np.float32
        ok = (gb["prim"] != MISS) & (z > 0) & np.isfinite(z)
        code = np.where(ok, np.where(ok, c, f32(1.0)).astype(np.int64) + 1, 1)
    return code


def code_of_depth(z, near):
    """The code of a hit at depth z (the arithmetic of pixel_codes on a depth alone), for the tests of the code itself."""
    z = np.asarray(z, np.float32)
    gb = dict(prim=np.zeros(z.shape, np.uint32), position=np.stack([np.zeros_like(z), np.zeros_like(z), z, np.ones_like(z)], axis=-1))
    return pixel_codes(gb, dict(eye=(0, 0, 0), U=(1, 0, 0), V=(0, 1, 0), W=(0, 0, 1)), near)      # (M = identity: z as given)


def depth_of_code(code, near):
    code = np.asarray(code, np.int64)
    with np.errstate(divide="ignore"):
        d = (f32(near) * f32(65534.0)) / np.maximum(code - 1, 0).astype(np.float32)
    return np.where(code == 1, f32(np.inf), d).astype(np.float32)


def pass_bytes(gw, gh):
    return (2 * gw * gh + 3) & ~3


def header(size, pas, cam, near, sequence=0):
    """-> (the 192 header bytes, the byte offset of every pass's codes, the packet's size in bytes)."""
    offs, at = [], HEADER_BYTES
    for gw, gh, *_ in pas:
        offs.append(at)
        at += pass_bytes(gw, gh)
    words = [MAGIC, VERSION, at, sequence & M32, size[0], size[1], len(pas), 0]
    for (gw, gh, fac, fill, ox, oy), off in zip(pas, offs):
        words += [gw, gh, fac, fill, ox, oy, off, 0]
    words += [0] * (32 - len(words))
    cam12 = [float(f32(c)) for k in ("eye", "U", "V", "W") for c in cam[k]]
    return struct.pack("<32I", *words) + struct.pack("<13f3I", *cam12, float(f32(near)), 0, 0, 0), offs, at


def texel_codes(codes, size, gaze, radii, uniform):
    """-> per pass the (gw * gh) int64 texel codes: the maximum over the owned pixels, 0 where none is owned."""
    pas = pk.passes(size, gaze, radii, uniform)
    own_p, own_l = pk.owners(size, gaze, radii, uniform)
    out = []
    for p, (gw, gh, *_) in enumerate(pas):
        sel = own_p == p
        tex = np.zeros(gw * gh, np.int64)
        np.maximum.at(tex, own_l[sel], codes[sel])
        out.append(tex)
    return out


def encode(gb, cam, near, size, gaze, radii, uniform, sequence=0):
    """-> the packet's bytes."""
    pas = pk.passes(size, gaze, radii, uniform)
    head, offs, total = header(size, pas, cam, near, sequence)
    out = bytearray(head)
    for tex in texel_codes(pixel_codes(gb, cam, near), size, gaze, radii, uniform):
        out += tex.astype("<u2").tobytes()
        out += bytes(-len(out) % 4)
    assert len(out) == total
    return bytes(out)


def parse(packet):
    """-> dict(bytes, sequence, width, height, passes: [(gw, gh, factor, fill, offx, offy, offset)], camera, near) or None: the
    checks of fovpt_packet_check_depth."""
    if len(packet) < HEADER_BYTES:
        return None
    w = struct.unpack("<32I", packet[:128])
    magic, version, nbytes, sequence, width, height, npass, res = w[:8]
    if magic != MAGIC or version != VERSION or nbytes > len(packet) or nbytes < HEADER_BYTES or res:
        return None
    width, height = (v - (1 << 32) if v >> 31 else v for v in (width, height))
    if not (1 <= width <= pk.MAX_DIM and 1 <= height <= pk.MAX_DIM and 1 <= npass <= 3):
        return None
    out, texels = [], 0
    for p in range(3):
        gw, gh, fac, fill, ox, oy, off, r = w[8 + 8 * p:16 + 8 * p]
        if p >= npass:
            if any(w[8 + 8 * p:16 + 8 * p]):
                return None
            continue
        texels += gw * gh
        if r or gw == 0 or gh == 0 or gw * gh > pk.MAX_TEXELS or texels > pk.MAX_TEXELS or fac == 0 or not 1 <= fill <= pk.MAX_FILL:
            return None
        if off < HEADER_BYTES or off % 4 or off + pass_bytes(gw, gh) > nbytes:
            return None
        out.append((gw, gh, fac, fill, ox, oy, off))
    cam12 = np.frombuffer(packet, "<f4", 12, 128)
    near = np.frombuffer(packet, "<f4", 1, 176)[0]
    if not np.isfinite(cam12).all() or any(struct.unpack("<3I", packet[180:192])):
        return None
    cam = dict(eye=tuple(cam12[0:3]), U=tuple(cam12[3:6]), V=tuple(cam12[6:9]), W=tuple(cam12[9:12]))
    if tr.camera_inverse(cam["U"], cam["V"], cam["W"]) is None or not (np.isfinite(near) and near > 0):
        return None
    return dict(bytes=nbytes, sequence=sequence, width=width, height=height, passes=out, camera=cam, near=f32(near))


def check(packet):
    return parse(packet) is not None


def decode(packet, out):
    """out: (h, w) float32, written in place where a texel reaches (the rest keeps its contents) and returned.  The packet must
    pass check()."""
    hd = parse(packet)
    assert hd is not None and out.shape == (hd["height"], hd["width"]) and out.dtype == np.float32
    w, h = hd["width"], hd["height"]
    best = np.full((h, w), -1, np.int64)                                  # pass << 40 | launch index of the last live texel
    texs = []
    for p, (gw, gh, fac, fill, ox, oy, off) in enumerate(hd["passes"]):
        tex = np.frombuffer(packet, "<u2", gw * gh, off).astype(np.int64).reshape(gh, gw)
        texs.append(tex)
        ly, lx = np.nonzero(tex)
        ix, iy = (lx * fac + ox) & M32, (ly * fac + oy) & M32
        key = (np.int64(p) << 40) | (ly * gw + lx)
        for v in range(fill):
            for u in range(fill):
                np.maximum.at(best, (np.minimum((iy + v) & M32, h - 1), np.minimum((ix + u) & M32, w - 1)), key)
    for p, (gw, *_ ) in enumerate(hd["passes"]):
        sel = (best >= 0) & ((best >> 40) == p)
        li = best[sel] & ((1 << 40) - 1)
        out[sel] = depth_of_code(texs[p][li // gw, li % gw], hd["near"])
    return out
