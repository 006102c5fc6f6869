"""numpy integer restatement of the coded frame packet (include/fovpt.h, FOVPT_PACKET_MAGIC_CODED; csrc/packet.hip,
k_packet_encode_coded and fetch_texel; csrc/packet_host.cpp): the definition device and host match bit for bit.  The texels and
the writers are those of tests/packet_ref.py.

    packet    magic "FVPC", version 1, the 128-byte header of packet_ref; the eighth word of a pass record is the pass's codec:
              RAW 0 -> 4 gw gh bytes of texels, BC1 1 -> 8 ceil(gw / 4) ceil(gh / 4) bytes of blocks, row-major by * ceil(gw / 4)
              + bx, block (bx, by) over texels (4 bx .. 4 bx + 3, 4 by .. 4 by + 3), texels beyond the grid dead; arrays back to back
    block     L = live texels (alpha != 0).  L empty: 00 00 00 00 ff ff ff ff.  lo / hi per channel over L; ref = the channel with
              the largest hi - lo (ties g, r, b); A gets hi_ref, B lo_ref; channel k != ref: s_k = sum_L (2 c_k - lo_k - hi_k)
              (2 c_ref - lo_ref - hi_ref); s_k < 0: A lo_k, B hi_k, else A hi_k, B lo_k.  q5(c) = (31 c + 127) // 255, q6(c) =
              (63 c + 127) // 255; a = q5(A_r) << 11 | q6(A_g) << 5 | q5(A_b), b likewise.  a == b: color0 = color1 = a; else all
              16 live: color0 = max, color1 = min (4 colours); else color0 = min, color1 = max (3 colours, index 3 transparent).
              Palette from e5(v) = v << 3 | v >> 2, e6(v) = v << 2 | v >> 4: P2 = (2 P0 + P1 + 1) // 3, P3 = (P0 + 2 P1 + 1) // 3,
              or P2 = (P0 + P1 + 1) // 2.  A live texel's index: the opaque entry with the least squared distance, ties lowest;
              a dead texel's: 3.  Bytes: color0, color1 LE16, then a LE32 word with texel (x, y) at bits 2 (4 y + x).
    decode    index 3 with color0 <= color1 -> 0x00000000, else 0xff000000 | b << 16 | g << 8 | r of the palette entry
    expand    every BC1 pass replaced by its decoded texels: a valid "FVPK" packet; NEAREST / SMOOTH of a coded packet are
              packet_ref's of expand(packet)."""
import struct

import numpy as np

import packet_ref as pk

MAGIC_CODED = 0x43505646
RAW, BC1, BY_FILL = 0, 1, 0xffffffff


def pass_bytes(gw, gh, codec):
    return 8 * ((gw + 3) // 4) * ((gh + 3) // 4) if codec == BC1 else 4 * gw * gh


def default_codecs(pas):
    """fovpt_packet_defaults on a frame's passes: BC1 where the fill is above 1."""
    return tuple(BC1 if p[3] > 1 else RAW for p in pas)


def header(size, pas, codecs, sequence=0):
    """-> (the 128 header bytes, the byte offset of every pass, the packet's size in bytes)."""
    assert len(codecs) == len(pas)
    offs, at = [], pk.HEADER_BYTES
    for (gw, gh, *_), k in zip(pas, codecs):
        offs.append(at)
        at += pass_bytes(gw, gh, k)
    words = [MAGIC_CODED, pk.VERSION, at, sequence & pk.M32, size[0], size[1], len(pas), 0]
    for (gw, gh, fac, fill, ox, oy), off, k in zip(pas, offs, codecs):
        words += [gw, gh, fac, fill, ox, oy, off, k]
    words += [0] * (32 - len(words))
    return struct.pack("<32I", *words), offs, at


def _q5(c):
    return (31 * c + 127) // 255


def _q6(c):
    return (63 * c + 127) // 255


def _expand565(c):
    """565 codes (n,) -> (n, 3) r, g, b."""
    r, g, b = c >> 11, (c >> 5) & 63, c & 31
    return np.stack([r << 3 | r >> 2, g << 2 | g >> 4, b << 3 | b >> 2], -1)


def _palette(c0, c1):
    """-> (n, 4, 3) palette entries and (n,) whether the block has four colours (color0 > color1)."""
    P0, P1 = _expand565(c0), _expand565(c1)
    four = c0 > c1
    f = four[:, None]
    P2 = np.where(f, (2 * P0 + P1 + 1) // 3, (P0 + P1 + 1) // 2)
    P3 = np.where(f, (P0 + 2 * P1 + 1) // 3, 0)
    return np.stack([P0, P1, P2, P3], 1), four


def encode_blocks(tex):
    """tex: (gh, gw) texels -> (bh * bw, 2) uint32 words of the BC1 blocks (color0 | color1 << 16, the indices)."""
    tex = np.asarray(tex, np.int64)
    gh, gw = tex.shape
    bh, bw = (gh + 3) // 4, (gw + 3) // 4
    pad = np.zeros((4 * bh, 4 * bw), np.int64)
    pad[:gh, :gw] = tex
    # (n, 16): texel (x, y) of a block at 4 y + x
    t = pad.reshape(bh, 4, bw, 4).transpose(0, 2, 1, 3).reshape(bh * bw, 16)
    n = len(t)
    live = (t >> 24) != 0
    c = np.stack([t & 0xff, (t >> 8) & 0xff, (t >> 16) & 0xff], -1)                 # (n, 16, 3)
    lv = live[:, :, None]
    lo = np.where(lv, c, 255).min(1)
    hi = np.where(lv, c, 0).max(1)                                                 # (n, 3); an all-dead block: lo 255, hi 0 (unused)
    ext = hi - lo
    ref = np.where((ext[:, 1] >= ext[:, 0]) & (ext[:, 1] >= ext[:, 2]), 1, np.where(ext[:, 0] >= ext[:, 2], 0, 2))
    d = np.where(lv, 2 * c - (lo + hi)[:, None, :], 0)                             # (n, 16, 3)
    dref = np.take_along_axis(d, ref[:, None, None], 2)                            # (n, 16, 1)
    s = (d * dref).sum(1)                                                          # (n, 3)
    assert np.abs(s).max(initial=0) < 1 << 31
    flip = (s < 0) & (np.arange(3)[None, :] != ref[:, None])
    A, B = np.where(flip, lo, hi), np.where(flip, hi, lo)
    a = _q5(A[:, 0]) << 11 | _q6(A[:, 1]) << 5 | _q5(A[:, 2])
    b = _q5(B[:, 0]) << 11 | _q6(B[:, 1]) << 5 | _q5(B[:, 2])
    four = (a != b) & live.all(1)
    c0 = np.where(four, np.maximum(a, b), np.minimum(a, b))
    c1 = np.where(four, np.minimum(a, b), np.maximum(a, b))
    pal, four2 = _palette(c0, c1)
    assert np.array_equal(four, four2)
    dist = ((c[:, :, None, :] - pal[:, None, :, :]) ** 2).sum(-1)                  # (n, 16, 4)
    dist[:, :, 3] = np.where(four[:, None], dist[:, :, 3], 1 << 40)                # (3 colours: entry 3 is not opaque)
    idx = np.where(live, dist.argmin(2), 3)                                        # (argmin: the first of equals)
    bits = (idx << (2 * np.arange(16))[None, :]).sum(1)
    dead = ~live.any(1)
    w0 = np.where(dead, 0, c0 | c1 << 16)
    w1 = np.where(dead, 0xffffffff, bits)
    return np.stack([w0, w1], -1).astype(np.uint32).reshape(n, 2)


def decode_blocks(words, gw, gh):
    """(bh * bw, 2) block words -> (gh, gw) texels."""
    words = np.asarray(words, np.int64).reshape(-1, 2)
    bh, bw = (gh + 3) // 4, (gw + 3) // 4
    assert len(words) == bh * bw
    c0, c1 = words[:, 0] & 0xffff, words[:, 0] >> 16
    pal, four = _palette(c0, c1)
    idx = (words[:, 1][:, None] >> (2 * np.arange(16))[None, :]) & 3               # (n, 16)
    rgb = np.take_along_axis(pal, idx[:, :, None], 1)                              # (n, 16, 3)
    val = 0xff000000 | rgb[:, :, 2] << 16 | rgb[:, :, 1] << 8 | rgb[:, :, 0]
    val = np.where((idx == 3) & ~four[:, None], 0, val)
    full = val.reshape(bh, bw, 4, 4).transpose(0, 2, 1, 3).reshape(4 * bh, 4 * bw)
    return full[:gh, :gw]


def transcode(raw_packet, codecs):
    """An "FVPK" packet (packet_ref.encode) -> the coded packet with those codecs per pass."""
    hd = pk.parse(raw_packet)
    assert hd is not None
    pas = [P[:6] for P in hd["passes"]]
    head, offs, total = header((hd["width"], hd["height"]), pas, codecs, hd["sequence"])
    out = bytearray(head)
    for P, k in zip(hd["passes"], codecs):
        tex = pk._texels(raw_packet, P)
        out += encode_blocks(tex).astype("<u4").tobytes() if k == BC1 else tex.astype("<u4").tobytes()
    assert len(out) == total
    return bytes(out)


def encode(image, size, gaze, radii, uniform, codecs=None, sequence=0):
    """image: (h, w) uint32 rgba8 -> the coded packet's bytes.  codecs: per pass, None: default_codecs."""
    raw = pk.encode(image, size, gaze, radii, uniform, sequence)
    if codecs is None:
        codecs = default_codecs(pk.passes(size, gaze, radii, uniform))
    return transcode(raw, tuple(codecs)[:len(pk.parse(raw)["passes"])])


def parse(packet):
    """-> dict(bytes, sequence, width, height, passes: [(gw, gh, factor, fill, offx, offy, offset)], codecs) or None: the checks
    of fovpt_packet_check on a coded packet."""
    if len(packet) < pk.HEADER_BYTES:
        return None
    w = struct.unpack("<32I", packet[:pk.HEADER_BYTES])
    magic, version, nbytes, sequence, width, height, npass, res = w[:8]
    if magic != MAGIC_CODED or version != pk.VERSION or nbytes > len(packet) or nbytes < pk.HEADER_BYTES or res:
        return None
    if not (1 <= width <= pk.MAX_DIM and 1 <= height <= pk.MAX_DIM and 1 <= npass <= 3):
        return None
    out, codecs, texels = [], [], 0
    for p in range(3):
        gw, gh, fac, fill, ox, oy, off, k = w[8 + 8 * p:16 + 8 * p]
        if p >= npass:
            if any(w[8 + 8 * p:16 + 8 * p]):
                return None
            continue
        texels += gw * gh
        if k not in (RAW, BC1) or gw == 0 or gh == 0 or texels > pk.MAX_TEXELS or fac == 0 or not 1 <= fill <= pk.MAX_FILL:
            return None
        if off < pk.HEADER_BYTES or off % 4 or off + pass_bytes(gw, gh, k) > nbytes:
            return None
        out.append((gw, gh, fac, fill, ox, oy, off))
        codecs.append(k)
    return dict(bytes=nbytes, sequence=sequence, width=width, height=height, passes=out, codecs=codecs)


def check(packet):
    """Either format."""
    return pk.check(packet) or parse(packet) is not None


def expand(packet):
    """A coded packet -> the "FVPK" packet with every BC1 pass decoded."""
    hd = parse(packet)
    assert hd is not None
    pas = [P[:6] for P in hd["passes"]]
    head, _, total = pk.header((hd["width"], hd["height"]), pas, hd["sequence"])
    out = bytearray(head)
    for (gw, gh, *_, off), k in zip(hd["passes"], hd["codecs"]):
        if k == BC1:
            words = np.frombuffer(packet, "<u4", 2 * ((gw + 3) // 4) * ((gh + 3) // 4), off)
            out += decode_blocks(words, gw, gh).astype("<u4").tobytes()
        else:
            out += packet[off:off + 4 * gw * gh]
    assert len(out) == total
    return bytes(out)


def decode(packet, mode, out):
    """Either format; out as packet_ref.decode's."""
    return pk.decode(packet if pk.check(packet) else expand(packet), mode, out)
