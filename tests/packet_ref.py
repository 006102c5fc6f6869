"""numpy integer restatement of the foveated frame packet (include/fovpt.h, fovpt_packet_*; csrc/packet.hip and
csrc/packet_host.cpp): the definition the device encoder, the device decoder and the host decoder match bit for bit.

    layout    128-byte header, then one rgba8 texel array per pass (launch order), row-major ly * gw + lx, back to back; all
              values little endian
    header    magic "FVPK", version 1, bytes (the whole packet), sequence, width, height, npass, 0, then three 32-byte pass
              records {gw, gh, factor, fill, offx, offy, texels (byte offset), 0}; unused records are zero
    encode    a launch index owns the pixels whose last writer it is (reconstruct_ref.writers); n owned pixels:
              n == 0 -> 0x00000000, else r, g, b = (sum + n // 2) // n of the owned pixels' codes and alpha 0xff
    NEAREST   texels with alpha != 0 write their fill x fill block, pixel min((l * factor + off + u) mod 2^32, dim - 1) per
              axis, in pass order and within a pass ascending (ly, lx); later writes win; other pixels keep what out held
    SMOOTH    a pixel whose NEAREST texel has fill == factor > 1 and whose anchor (ix, iy) satisfies 0 <= x - ix < fill,
              0 <= y - iy < fill is regular: dx = 2 (x - ix) + 1 - fill, sx = 1 if dx > 0 else -1, weights |dx| (neighbour) and
              2 fill - |dx| (own), the same along y; taps (lx, ly), (lx + sx, ly), (lx, ly + sy), (lx + sx, ly + sy) of the same
              pass, weighted by the products; a tap counts inside the grid with alpha != 0 (the own tap always counts); each
              of r, g, b is (sum w c + W // 2) // W over the counted taps, alpha 0xff.  Other pixels: NEAREST."""
import struct

import numpy as np

import reconstruct_ref as rr

MAGIC, VERSION, HEADER_BYTES, SLOTS = 0x4b505646, 1, 128, 4
NEAREST, SMOOTH = 0, 1
MAX_DIM, MAX_TEXELS, MAX_FILL = 16384, 1 << 26, 8
M32 = 0xffffffff


def passes(size, gaze, radii, uniform):
    """The pass records of the frame as rendered: (gw, gh, factor, fill, offx, offy) in launch order."""
    r_inner, r_outer = radii if radii is not None else (0, 0)
    return [tuple(int(v) for v in p[:6]) for p in rr.frame_passes(size[0], size[1], gaze, r_inner, r_outer, uniform)]


def header(size, pas, sequence=0):
    """-> (the 128 header bytes, the texel byte offset of every pass, the packet's size in bytes)."""
    offs, at = [], HEADER_BYTES
    for gw, gh, *_ in pas:
        offs.append(at)
        at += 4 * gw * gh
    words = [MAGIC, VERSION, at, sequence & M32, size[0], size[1], len(pas), 0]
    for (gw, gh, fac, fill, ox, oy), off in zip(pas, offs):
        words += [gw, gh, fac, fill, ox, oy, off, 0]
    words += [0] * (32 - len(words))
    return struct.pack("<32I", *words), offs, at


def owners(size, gaze, radii, uniform):
    """Per pixel its last writer's pass (-1: none) and launch index ly * gw + lx within that pass."""
    w, h = size
    r_inner, r_outer = radii if radii is not None else (0, 0)
    _, pas, ax, ay = rr.writers(w, h, gaze, r_inner, r_outer, uniform)
    li = np.zeros((h, w), np.int64)
    for p, (gw, gh, fac, fill, ox, oy) in enumerate(passes(size, gaze, radii, uniform)):
        sel = pas == p
        lx = ((ax[sel] - ox) & M32) // fac              # (anchor = (l * factor + off) mod 2^32 and l * factor < 2^32)
        ly = ((ay[sel] - oy) & M32) // fac
        assert (lx < gw).all() and (ly < gh).all()
        li[sel] = ly * gw + lx
    return pas, li


def encode(image, size, gaze, radii, uniform, sequence=0):
    """image: (h, w) uint32 rgba8 -> the packet's bytes."""
    w, h = size
    image = np.asarray(image, np.uint32).reshape(h, w)
    pas = passes(size, gaze, radii, uniform)
    head, offs, total = header(size, pas, sequence)
    own_p, own_l = owners(size, gaze, radii, uniform)
    out = bytearray(head)
    for p, (gw, gh, *_) in enumerate(pas):
        sel = own_p == p
        n = np.zeros(gw * gh, np.int64)
        np.add.at(n, own_l[sel], 1)
        tex = np.zeros(gw * gh, np.int64)
        live = n > 0
        d = np.where(live, n, 1)
        for k in range(3):
            s = np.zeros(gw * gh, np.int64)
            np.add.at(s, own_l[sel], ((image[sel] >> (8 * k)) & 0xff).astype(np.int64))
            tex |= ((s + d // 2) // d) << (8 * k)
        tex = np.where(live, tex | (0xff << 24), 0)
        out += tex.astype("<u4").tobytes()
    assert len(out) == total
    return bytes(out)


def parse(packet):
    """-> dict(bytes, sequence, width, height, passes: [(gw, gh, factor, fill, offx, offy, texels)]) or None: the checks of
    fovpt_packet_check."""
    if len(packet) < HEADER_BYTES:
        return None
    w = struct.unpack("<32I", packet[:HEADER_BYTES])
    magic, version, nbytes, sequence, width, height, npass, res = w[:8]
    if magic != MAGIC or version != VERSION or nbytes > len(packet) or nbytes < HEADER_BYTES or res:
        return None
    if not (1 <= width <= MAX_DIM and 1 <= height <= MAX_DIM and 1 <= npass <= 3):
        return None
    out, texels = [], 0
    for p in range(3):
        gw, gh, fac, fill, ox, oy, off, r = w[8 + 8 * p:16 + 8 * p]
        if p >= npass:
            if any(w[8 + 8 * p:16 + 8 * p]):
                return None
            continue
        texels += gw * gh
        if r or gw == 0 or gh == 0 or texels > MAX_TEXELS or fac == 0 or not 1 <= fill <= MAX_FILL:
            return None
        if off < HEADER_BYTES or off % 4 or off + 4 * gw * gh > nbytes:
            return None
        out.append((gw, gh, fac, fill, ox, oy, off))
    return dict(bytes=nbytes, sequence=sequence, width=width, height=height, passes=out)


def check(packet):
    return parse(packet) is not None


def _texels(packet, P):
    gw, gh, *_, off = P
    return np.frombuffer(packet, "<u4", gw * gh, off).astype(np.int64).reshape(gh, gw)


def _nearest_map(packet, hd):
    """Per pixel the key (pass << 40 | launch index) of the texel that writes it last, -1: none."""
    w, h = hd["width"], hd["height"]
    best = np.full((h, w), -1, np.int64)
    for p, P in enumerate(hd["passes"]):
        gw, gh, fac, fill, ox, oy, _ = P
        tex = _texels(packet, P)
        ly, lx = np.nonzero(tex >> 24)
        ix, iy = (lx * fac + ox) & M32, (ly * fac + oy) & M32
        key = (np.int64(p) << 40) | (ly * gw + lx)
        for v in range(fill):
            for u in range(fill):
                np.maximum.at(best, (np.minimum((iy + v) & M32, h - 1), np.minimum((ix + u) & M32, w - 1)), key)
    return best


def decode(packet, mode, out):
    """out: (h, w) uint32, written in place where a texel reaches (the rest keeps its contents) and returned.  The packet must
    pass check()."""
    hd = parse(packet)
    assert hd is not None and mode in (NEAREST, SMOOTH) and out.shape == (hd["height"], hd["width"]) and out.dtype == np.uint32
    best = _nearest_map(packet, hd)
    Y, X = np.mgrid[0:hd["height"], 0:hd["width"]]
    for p, P in enumerate(hd["passes"]):
        gw, gh, fac, fill, ox, oy, _ = P
        tex = _texels(packet, P)
        sel = (best >= 0) & ((best >> 40) == p)
        li = best[sel] & ((1 << 40) - 1)
        lx, ly = li % gw, li // gw
        val = tex[ly, lx]
        if mode == SMOOTH and fill == fac and fill > 1:
            x, y = X[sel], Y[sel]
            rx, ry = x - ((lx * fac + ox) & M32), y - ((ly * fac + oy) & M32)
            reg = (rx >= 0) & (rx < fill) & (ry >= 0) & (ry < fill)
            dx, dy = 2 * rx + 1 - fill, 2 * ry + 1 - fill
            sx, sy = np.where(dx > 0, 1, -1), np.where(dy > 0, 1, -1)
            wx = (2 * fill - np.abs(dx), np.abs(dx))
            wy = (2 * fill - np.abs(dy), np.abs(dy))
            W = np.zeros(len(li), np.int64)
            acc = [np.zeros(len(li), np.int64) for _ in range(3)]
            for j in (0, 1):
                for i in (0, 1):
                    tx, ty = lx + i * sx, ly + j * sy
                    inside = (tx >= 0) & (tx < gw) & (ty >= 0) & (ty < gh)
                    c = tex[np.clip(ty, 0, gh - 1), np.clip(tx, 0, gw - 1)]
                    wt = np.where(inside & ((c >> 24) != 0), wx[i] * wy[j], 0)
                    W += wt
                    for k in range(3):
                        acc[k] += wt * ((c >> (8 * k)) & 0xff)
            sm = np.full(len(li), 0xff << 24, np.int64)
            for k in range(3):
                sm |= ((acc[k] + W // 2) // np.maximum(W, 1)) << (8 * k)
            val = np.where(reg, sm, val)
        out[sel] = val.astype(np.uint32)
    return out
