"""The depth packet "FVPD" without a GPU: the code itself (monotone, its error bound, saturation, the order-free texel maximum),
the host decoder and fovpt_packet_check_depth of both libraries against tests/packet_depth_ref.py bit for bit, every listed
rejection by a one-field mutation, a sanitizer build of csrc/packet_host.cpp fed those and random damage, and the ABI."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import header_layout
import packet_depth_ref as pd
import packet_ref as pk
from fovpathtracing_optixcodelatest_amd import abi, abi_depth, lib, renderer
from packet_cases import IDS, SHAPES, random_frame
from packet_depth_cases import JUNK_DEPTH, camera_dict, junk_depth, mutations, synthetic_gbuffer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
f32 = np.float32


@pytest.fixture(scope="module")
def libs():
    """(name, library) for the host-only loader library and for libfovpt.so: both carry the depth packet's checks and decoder."""
    lib.build()
    L = C.CDLL(lib.LOADER_SO_PATH)
    lib._declare_loader(L)
    lib._declare_packet_host(L)
    return [("libfovpt_loader.so", L), ("libfovpt.so", lib.load())]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host_decode(L, packet, out):
    return L.fovpt_packet_decode_depth_host(packet, len(packet), out.ctypes.data, out.shape[1], out.shape[0])


def synthetic_packet(k, seed, near=pd.DEFAULT_NEAR, sequence=0):
    size, gaze, radii, uniform = SHAPES[k]
    cam = camera_dict(size)
    gb = synthetic_gbuffer(size, cam, seed)
    return gb, cam, pd.encode(gb, cam, near, size, gaze, radii, uniform, sequence)


# ---- 1. the code ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("near", [0.05, 0.1, 1.0])
def test_the_code_is_monotone_bounded_and_saturates(near):
    rng = np.random.default_rng(3)
    z = np.sort(np.exp(rng.uniform(np.log(1e-3), np.log(1e7), 200000)).astype(np.float32))
    code = pd.code_of_depth(z, near)
    assert ((code >= 2) & (code <= 65535)).all()
    assert (np.diff(code) <= 0).all()                                     # nearer never gets a smaller code
    # In the reciprocal domain: c = floor(fl(fl(fl(near / z) * 65534) + 0.5)) has three binary32 roundings ahead of the floor --
    # the quotient, the product and the sum with 0.5 --, each within u = 2^-24 relative, on values of at most t + 0.5 with
    # t = 65534 near / z exact.  floor moves its argument by less than 1 downwards, so |c - t| <= 0.5 + the roundings, which
    # are at most t (2 u + u^2) for the first two and (t (1 + u)^2 + 0.5) u for the third: below 4 u (t + 1).
    t = 65534.0 * float(f32(near)) / z.astype(np.float64)
    open_ = (t >= 1.0) & (t <= 65534.0)                                   # not saturated
    err = np.abs((code[open_] - 1) - t[open_])
    bound = 0.5 + 4.0 * 2.0 ** -24 * (t[open_] + 1.0)
    assert open_.sum() > 50000 and (err <= bound).all(), float((err - bound).max())
    assert bound.max() < 0.52
    # saturation at both ends, and the values next to them
    n = f32(near)
    assert pd.code_of_depth(np.array([n, n / f32(2), f32(1e-30), np.nextafter(f32(0), f32(1))], np.float32), near).tolist() == [65535] * 4
    assert pd.code_of_depth(np.array([n * f32(1e6), f32(3e38)], np.float32), near).tolist() == [2, 2]
    assert pd.code_of_depth(np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf], np.float32), near).tolist() == [1] * 6
    # the decoder's depth of a code is within half a step of the reciprocal
    d = pd.depth_of_code(np.arange(1, 65536), near)
    assert np.isinf(d[0]) and (np.diff(d[1:]) < 0).all() and d.dtype == np.float32
    assert abs(float(d[-1]) - float(n)) <= float(np.spacing(n))           # (code 65535 is near, up to the two roundings)


def test_the_texel_maximum_does_not_depend_on_the_pixel_order():
    size, gaze, radii, uniform = SHAPES[0]
    cam = camera_dict(size)
    gb = synthetic_gbuffer(size, cam, 5)
    codes = pd.pixel_codes(gb, cam, 0.1)
    want = pd.texel_codes(codes, size, gaze, radii, uniform)
    own_p, own_l = pk.owners(size, gaze, radii, uniform)
    rng = np.random.default_rng(1)
    for _ in range(3):
        order = rng.permutation(codes.size)
        for p, tex in enumerate(want):
            got = np.zeros_like(tex)
            for s in order:                                               # one pixel at a time, in this order
                y, x = divmod(int(s), size[0])
                if own_p[y, x] == p:
                    got[own_l[y, x]] = max(got[own_l[y, x]], codes[y, x])
            assert np.array_equal(got, tex)


# ---- 2. the host decoder and the check against the restatement ------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_host_decoder_matches_the_restatement(libs, k):
    size, gaze, radii, uniform = SHAPES[k]
    gb, cam, packet = synthetic_packet(k, 20 + k, sequence=9)
    # the case holds what it is for: sky, the farthest and the nearest code, and a texel that owns sky and hit pixels
    codes = pd.pixel_codes(gb, cam, pd.DEFAULT_NEAR)
    assert {1, 2, 65535} <= set(np.unique(codes).tolist())
    own_p, own_l = pk.owners(size, gaze, radii, uniform)
    texels = pd.texel_codes(codes, size, gaze, radii, uniform)
    if not uniform:                                                       # (FOV_OFF: every texel is one pixel)
        mixed = 0
        for p, tex in enumerate(texels):
            sel = own_p == p
            sky, hit = np.zeros(tex.size, bool), np.zeros(tex.size, bool)
            sky[own_l[sel & (codes == 1)]] = True
            hit[own_l[sel & (codes > 1)]] = True
            mixed += int((sky & hit).sum())
            assert (tex[sky & hit] > 1).all() and (tex[sky & ~hit] == 1).all()      # sky wins only where every owned pixel is sky
        assert mixed > 0
    hd = pd.parse(packet)
    assert hd is not None and len(packet) == hd["bytes"] and len(packet) % 4 == 0 and hd["sequence"] == 9
    assert packet[:4] == b"FVPD" and [P[6] for P in hd["passes"]][0] == 192
    want = pd.decode(packet, junk_depth(size))
    written = pk.owners(size, gaze, radii, uniform)[0] >= 0
    assert (want[~written] == JUNK_DEPTH).all() and (want[written] > 0).all() and np.isinf(want).any()
    for name, L in libs:
        assert L.fovpt_packet_check_depth(packet, len(packet)) == 0, name
        got = junk_depth(size)
        assert host_decode(L, packet, got) == 0, name
        assert np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).sum()))
        # the colour entry points refuse it
        assert L.fovpt_packet_check(packet, len(packet)) == E_INVALID
        assert L.fovpt_packet_decode_host(packet, len(packet), 0, got.ctypes.data, size[0], size[1]) == E_INVALID
    assert np.array_equal(bits(renderer.decode_depth_packet(packet, size, out=junk_depth(size))), bits(want))
    assert renderer.decode_depth_packet(packet).shape == (size[1], size[0])
    # a colour packet is no depth packet
    colour = pk.encode(random_frame(size, 1), size, gaze, radii, uniform)
    for name, L in libs:
        assert L.fovpt_packet_check_depth(colour, len(colour)) == E_INVALID


def test_a_packet_spelled_out():
    """2 x 2, FOV_OFF, the identity camera: every byte by hand."""
    cam = dict(eye=(0.0, 0.0, 0.0), U=(1.0, 0.0, 0.0), V=(0.0, 1.0, 0.0), W=(0.0, 0.0, 1.0))
    pos = np.zeros((2, 2, 4), np.float32)
    pos[..., 2] = [[0.1, 0.2], [1e9, -1.0]]
    gb = dict(prim=np.array([[0, 0], [0, 0xffffffff]], np.uint32), position=pos)
    got = pd.encode(gb, cam, 0.1, (2, 2), (0, 0), None, True, sequence=7)
    want = struct.pack("<8I", 0x44505646, 1, 200, 7, 2, 2, 1, 0) + struct.pack("<8I", 2, 2, 1, 1, 0, 0, 192, 0) + bytes(64)
    want += struct.pack("<13f3I", 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, float(f32(0.1)), 0, 0, 0)
    want += struct.pack("<4H", 65535, 32768, 2, 1)                        # near / z = 1, 0.5, ~0, sky
    assert got == want
    out = pd.decode(got, np.zeros((2, 2), np.float32))
    assert out[0, 0] == f32(0.1) and out[1, 1] == np.inf and out[1, 0] == f32(0.1) * f32(65534.0)
    # an odd number of texels: two bytes of zero padding
    odd = pd.encode(dict(prim=gb["prim"][:1, :1].repeat(3, 1), position=pos[:1, :1].repeat(3, 1)), cam, 0.1, (3, 1), (0, 0), None, True)
    assert len(odd) == 200 and odd[192:] == struct.pack("<4H", 65535, 65535, 65535, 0)


# ---- 3. untrusted input ---------------------------------------------------------------------------------------------------------------
def _cases():
    """(valid packets, [(label, bytes, check must refuse, the size of the packet it was made from)])"""
    valid, bad = [], []
    for k in (0, 2, 5):                                                   # three passes, wrapped offsets, one pass
        packet = synthetic_packet(k, 40 + k)[2]
        valid.append(packet)
        bad += [("%s: %s" % (IDS[k], label), m, not label.startswith("another"), SHAPES[k][0]) for label, m in mutations(packet)]
    p0 = valid[0]
    bad += [("truncated to %d" % n, p0[:n], True, SHAPES[0][0]) for n in range(0, len(p0), 4)]
    return valid, bad


def test_every_rejection_by_a_one_field_mutation(libs):
    valid, bad = _cases()
    assert len(bad) > 500
    for name, L in libs:
        for packet in valid:
            assert L.fovpt_packet_check_depth(packet, len(packet)) == 0
        for label, m, refused, size in bad:
            assert pd.check(m) == (not refused), label
            assert L.fovpt_packet_check_depth(m, len(m)) == (E_INVALID if refused else 0), (name, label)
            out = junk_depth(size)
            assert host_decode(L, m, out) == E_INVALID, (name, label)     # ("another width": not the output's)
            assert (out == JUNK_DEPTH).all(), (name, label)
        packet, size = valid[0], SHAPES[0][0]
        out = junk_depth(size)
        assert L.fovpt_packet_decode_depth_host(packet, len(packet), None, size[0], size[1]) == E_INVALID
        assert L.fovpt_packet_decode_depth_host(None, len(packet), out.ctypes.data, size[0], size[1]) == E_INVALID
        assert L.fovpt_packet_check_depth(None, 4096) == E_INVALID
        assert L.fovpt_packet_decode_depth_host(packet, len(packet), out.ctypes.data, size[1], size[0]) == E_INVALID
        assert (out == JUNK_DEPTH).all()
        assert L.fovpt_packet_check_depth(packet + bytes(100), len(packet) + 100) == 0      # (more bytes than the packet: fine)
        assert b"fovpt_packet" in L.fovpt_last_error(None)
    with pytest.raises(lib.FovptError):
        renderer.decode_depth_packet(valid[0][:-4])
    with pytest.raises(lib.FovptError):
        renderer.decode_depth_packet(b"FVPD")


def test_untrusted_depth_packets_under_sanitizers(tmp_path):
    """csrc/packet_host.cpp in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer: the valid
    packets, every mutation and truncation above, and 200 seeded randomly damaged packets per file.  Every call returns FOVPT_OK
    or FOVPT_E_INVALID and the sanitizers stay silent."""
    exe = str(tmp_path / "packet_depth_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "fovpathtracing_optixcodelatest_amd", "csrc", "packet_host.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "packet_depth_host_main.cpp"), "-o", exe])
    valid, bad = _cases()
    files = []
    for k, packet in enumerate(valid):                                    # a file per valid packet: it and the cases made from it
        mine = [m for label, m, _, _ in bad if label.startswith(IDS[(0, 2, 5)[k]]) or (k == 0 and label.startswith("truncated"))]
        path = str(tmp_path / ("cases%d.bin" % k))
        with open(path, "wb") as f:
            for b in [packet] + mine:
                f.write(struct.pack("<I", len(b)) + b)
        files.append((path, 1 + len(mine)))
    res = subprocess.run([exe, "200"] + [p for p, _ in files], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    assert "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(files), res.stdout
    for (path, n), line in zip(files, lines):
        f = dict(kv.split("=") for kv in line.split()[1:])
        assert int(f["packets"]) == n and int(f["bad"]) == 0 and int(f["fuzzed"]) == 200, line
        assert 1 <= int(f["valid"]) <= 3                                   # (the packet, and "another width / height")
        assert 0 < int(f["fuzzed_valid"]) < 200, line                      # (the damage reaches both outcomes)


# ---- 4. the ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_mirrors_are_pinned_to_the_header():
    fields = [("fovpt_packet_depth_config", abi_depth.PacketDepthConfig, {}), ("fovpt_packet_depth_header", abi_depth.PacketDepthHeader, {})]
    lines, consts = header_layout.probe([(cname, [n for n, _ in T._fields_], ren) for cname, T, ren in fields],
                                        ("FOVPT_PACKET_MAGIC_DEPTH", "FOVPT_PACKET_DEPTH_HEADER_BYTES", "FOVPT_PACKET_VERSION"))
    for (cname, T, _), got in zip(fields, lines):
        assert got[0] == C.sizeof(T) == {"fovpt_packet_depth_config": 16, "fovpt_packet_depth_header": 192}[cname]
        assert got[1:] == [getattr(T, n).offset for n, _ in T._fields_]
    assert consts == [abi_depth.PACKET_MAGIC_DEPTH, abi_depth.PACKET_DEPTH_HEADER_BYTES, abi.PACKET_VERSION]
    assert (pd.MAGIC, pd.HEADER_BYTES, pd.VERSION) == (abi_depth.PACKET_MAGIC_DEPTH, abi_depth.PACKET_DEPTH_HEADER_BYTES, abi.PACKET_VERSION)
    h = abi_depth.PacketDepthHeader.from_packet(synthetic_packet(0, 1, sequence=3)[2])
    assert (h.base.magic, h.base.sequence, h.base.npass, h.base.passes[0].texels) == (pd.MAGIC, 3, 3, 192) and h.near == pd.DEFAULT_NEAR


def test_defaults_symbols_and_the_entry_points_without_a_context(libs):
    text = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    full = dict(libs)["libfovpt.so"]
    loader = C.CDLL(lib.LOADER_SO_PATH)
    for n in ("fovpt_packet_describe_depth", "fovpt_packet_encode_depth", "fovpt_packet_submit_depth", "fovpt_packet_check_depth",
              "fovpt_packet_decode_depth_host", "fovpt_packet_decode_depth", "fovpt_warp_depth"):
        assert ("int %s(" % n) in text and n in lib.EXPORTS and hasattr(full, n), n
    for n in ("fovpt_packet_depth_defaults", "fovpt_packet_check_depth", "fovpt_packet_decode_depth_host"):
        assert n in lib.PACKET_HOST_EXPORTS and hasattr(loader, n), n
    for n in ("fovpt_packet_encode_depth", "fovpt_packet_decode_depth", "fovpt_warp_depth"):
        assert not hasattr(loader, n), n                                  # (the context's entry points need the device)
    for _, L in libs:
        cfg = abi_depth.PacketDepthConfig(near=5.0)
        cfg._reserved[1] = 9
        L.fovpt_packet_depth_defaults(C.byref(cfg))
        assert cfg.near == f32(0.1) and list(cfg._reserved) == [0, 0, 0]
        L.fovpt_packet_depth_defaults(None)
    assert full.fovpt_packet_describe_depth(None, None, None, 0, None) == E_INVALID
    assert full.fovpt_packet_encode_depth(None, None, None, None, 0, None) == E_INVALID
    assert full.fovpt_packet_submit_depth(None, None, None, None, 0, None) == E_INVALID
    assert full.fovpt_packet_decode_depth(None, None, None, None) == E_INVALID
    assert full.fovpt_warp_depth(None, 4, 4, None, None, None, None, None, None, None, None, None) == E_INVALID
    shim = open(os.path.join(ROOT, "include", "SimplePathtracer.h")).read()
    for n in ("submitDepthPacket", "decodeDepthPacket", "warpDepth"):
        assert n in shim, n
