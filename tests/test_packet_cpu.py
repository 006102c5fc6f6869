"""The foveated frame packet without a GPU: the reference's sizes on hand cases, the host decoder (csrc/packet_host.cpp, in both
libraries) against tests/packet_ref.py bit for bit, the wire format pinned by a golden packet, untrusted input -- every listed
rejection by a one-field mutation, every truncation, and a sanitizer build fed those plus seeded random mutations -- and the ABI."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import header_layout
import packet_ref as pk
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer
from packet_cases import IDS, JUNK, SHAPES, junk_canvas, mutations, random_frame, synthetic_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E_INVALID = -1


@pytest.fixture(scope="module")
def libs():
    """(name, library) for the host-only loader library and for libfovpt.so: both carry the decoder."""
    lib.build()
    L = C.CDLL(lib.LOADER_SO_PATH)
    lib._declare_loader(L)
    lib._declare_packet_host(L)
    return [("libfovpt_loader.so", L), ("libfovpt.so", lib.load())]


def host_decode(L, packet, mode, out):
    rc = L.fovpt_packet_decode_host(packet, len(packet), mode, out.ctypes.data, out.shape[1], out.shape[0])
    return rc


# ---- 1. the reference on hand cases -----------------------------------------------------------------------------------------------
def test_reference_sizes_and_a_packet_spelled_out():
    assert pk.header((64, 48), pk.passes((64, 48), (32, 24), (6, 14), False))[2] == 2704
    assert pk.header((1920, 1080), pk.passes((1920, 1080), (960, 540), (74, 241), False))[2] == 844724      # 128 + 4 * 211 149
    assert pk.header((1920, 1080), pk.passes((1920, 1080), (960, 540), (148, 482), False))[2] == 128 + 4 * (480 * 270 + 484 ** 2 + 298 ** 2)
    img = np.array([[0xff010203, 0x00000000], [0x12345678, 0xffffffff]], np.uint32)
    got = pk.encode(img, (2, 2), (0, 0), None, True, sequence=7)
    want = struct.pack("<8I", 0x4b505646, 1, 144, 7, 2, 2, 1, 0) + struct.pack("<8I", 2, 2, 1, 1, 0, 0, 128, 0) + bytes(64)
    want += struct.pack("<4I", 0xff010203, 0xff000000, 0xff345678, 0xffffffff)      # every pixel is owned: alpha 0xff, the rest as it is
    assert got[:4] == b"FVPK" and got == want
    out = np.full((2, 2), JUNK, np.uint32)
    assert np.array_equal(pk.decode(got, pk.NEAREST, out), np.array([[0xff010203, 0xff000000], [0xff345678, 0xffffffff]], np.uint32))
    # averaging: the four periphery texels of an 8 x 8 frame, each over the pixels the inner passes leave it
    size, gaze, radii = (8, 8), (5, 5), (0, 1)
    img = random_frame(size, 1)
    pas, li = pk.owners(size, gaze, radii, False)
    packet = pk.encode(img, size, gaze, radii, False)
    counts = set()
    for t in range(4):
        mine = [int(v) for v in img[(pas == 0) & (li == t)]]
        n = len(mine)
        counts.add(n)
        want = 0 if n == 0 else 0xff000000 | sum(((sum((v >> (8 * k)) & 0xff for v in mine) + n // 2) // n) << (8 * k) for k in range(3))
        assert struct.unpack("<I", packet[128 + 4 * t:132 + 4 * t])[0] == want, t
    assert 16 in counts and len(counts) > 1                              # (a whole block, and one the fovea cuts into)


# ---- 2. the host decoder against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_host_decoder_matches_the_reference(libs, shape):
    size, gaze, radii, uniform = shape
    raw, written = synthetic_raw(size, gaze, radii, uniform)
    assert written.any() and (uniform or size[0] % 4 == 0 or not written.all())
    frames = [("raw", raw), ("random", random_frame(size, 11))]
    for label, img in frames:
        packet = pk.encode(img, size, gaze, radii, uniform, sequence=5)
        assert pk.check(packet) and len(packet) == pk.parse(packet)["bytes"]
        for mode in (pk.NEAREST, pk.SMOOTH):
            want = pk.decode(packet, mode, junk_canvas(size))
            if label == "raw" and mode == pk.NEAREST:                    # the round trip, no pixel excluded
                assert np.array_equal(want[written], raw[written]) and (want[~written] == JUNK).all()
            assert (want[~written] == JUNK).all() and ((want[written] >> 24) == 0xff).all()
            for name, L in libs:
                assert L.fovpt_packet_check(packet, len(packet)) == 0
                got = junk_canvas(size)
                assert host_decode(L, packet, mode, got) == 0, (name, label, mode)
                assert np.array_equal(got, want), (name, label, mode, int((got != want).sum()))
        sm, ne = pk.decode(packet, pk.SMOOTH, junk_canvas(size)), pk.decode(packet, pk.NEAREST, junk_canvas(size))
        if label == "random" and not uniform:
            assert (sm != ne).mean() > 0.2                                # (SMOOTH does something)
        if uniform:
            assert np.array_equal(sm, ne)                                 # (fill 1: no pixel is regular)
    assert np.array_equal(renderer.decode_packet(packet, abi.PACKET_SMOOTH, size, out=junk_canvas(size)), sm)


# ---- 3. the wire format, pinned -----------------------------------------------------------------------------------------------------
def test_golden_packet(libs):
    packet = open(os.path.join(GOLDEN, "packet_v1_64x48.bin"), "rb").read()
    assert len(packet) == 2704
    size, gaze, radii, uniform = SHAPES[0]
    assert pk.encode(random_frame(size, 2024), size, gaze, radii, uniform, sequence=0x01020304) == packet
    h = abi.PacketHeader.from_packet(packet)
    assert (h.magic, h.version, h.bytes, h.sequence, h.width, h.height, h.npass) == (abi.PACKET_MAGIC, 1, 2704, 0x01020304, 64, 48, 3)
    assert [(p.gw, p.gh, p.factor, p.fill, p.texels) for p in h.passes] == [(16, 12, 4, 4, 128), (16, 16, 2, 2, 896), (14, 14, 1, 1, 1920)]
    for mode, name in ((pk.NEAREST, "nearest"), (pk.SMOOTH, "smooth")):
        want = np.fromfile(os.path.join(GOLDEN, "packet_v1_64x48_%s.bin" % name), "<u4").reshape(48, 64)
        assert np.array_equal(pk.decode(packet, mode, np.zeros((48, 64), np.uint32)), want)
        for _, L in libs:
            got = np.zeros((48, 64), np.uint32)
            assert host_decode(L, packet, mode, got) == 0 and np.array_equal(got, want)


# ---- 4. untrusted input ---------------------------------------------------------------------------------------------------------------
def _cases():
    """(valid packets, [(label, bytes, check must refuse, the size of the packet it was made from)])"""
    valid, bad = [], []
    for k in (0, 2, 5):                                                   # three passes, wrapped offsets, one pass
        size, gaze, radii, uniform = SHAPES[k]
        packet = pk.encode(random_frame(size, 3 + k), size, gaze, radii, uniform)
        valid.append(packet)
        bad += [("%s: %s" % (IDS[k], label), m, not label.startswith("another"), size) for label, m in mutations(packet)]
    p0 = valid[0]
    bad += [("truncated to %d" % n, p0[:n], True, SHAPES[0][0]) for n in range(0, len(p0), 4)]
    return valid, bad


def test_every_rejection_by_a_one_field_mutation(libs):
    valid, bad = _cases()
    assert len(valid[0]) == 2704 and len(bad) > 700
    for name, L in libs:
        for packet in valid:
            assert L.fovpt_packet_check(packet, len(packet)) == 0
        for label, m, refused, size in bad:
            assert pk.check(m) == (not refused), label
            assert L.fovpt_packet_check(m, len(m)) == (E_INVALID if refused else 0), (name, label)
            out = junk_canvas(size)
            for mode in (0, 1):
                assert host_decode(L, m, mode, out) == E_INVALID, (name, label, mode)      # ("another width": not the output's)
            assert (out == JUNK).all(), (name, label)
        packet, size = valid[0], (64, 48)
        out = junk_canvas(size)
        for mode in (-1, 2, 1 << 20):
            assert host_decode(L, packet, mode, out) == E_INVALID
        assert L.fovpt_packet_decode_host(packet, len(packet), 0, None, 64, 48) == E_INVALID
        assert L.fovpt_packet_decode_host(None, len(packet), 0, out.ctypes.data, 64, 48) == E_INVALID and L.fovpt_packet_check(None, 4096) == E_INVALID
        assert L.fovpt_packet_decode_host(packet, len(packet), 0, out.ctypes.data, 48, 64) == E_INVALID
        assert (out == JUNK).all()
        assert L.fovpt_packet_check(packet + bytes(100), len(packet) + 100) == 0      # (more bytes than the packet: fine)
        assert b"fovpt_packet" in L.fovpt_last_error(None)
    with pytest.raises(lib.FovptError):
        renderer.decode_packet(valid[0][:-4])
    with pytest.raises(lib.FovptError):
        renderer.decode_packet(b"FVPK")


def test_untrusted_packets_under_sanitizers(tmp_path):
    """csrc/packet_host.cpp in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer: the valid packets,
    every mutation and truncation above, and seeded random mutations.  Every call returns FOVPT_OK or FOVPT_E_INVALID and the
    sanitizers stay silent."""
    exe = str(tmp_path / "packet_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "fovpathtracing_optixcodelatest_amd", "csrc", "packet_host.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "packet_host_main.cpp"), "-o", exe])
    valid, bad = _cases()
    files = []
    for k, packet in enumerate(valid):                                    # a file per valid packet: it and the cases made from it
        mine = [m for label, m, _, _ in bad if label.startswith(IDS[(0, 2, 5)[k]]) or (k == 0 and label.startswith("truncated"))]
        path = str(tmp_path / ("cases%d.bin" % k))
        with open(path, "wb") as f:
            for b in [packet] + mine:
                f.write(struct.pack("<I", len(b)) + b)
        files.append((path, 1 + len(mine)))
    res = subprocess.run([exe, "3000"] + [p for p, _ in files], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    assert "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(files), res.stdout
    for (path, n), line in zip(files, lines):
        f = dict(kv.split("=") for kv in line.split()[1:])
        assert int(f["packets"]) == n and int(f["bad"]) == 0 and int(f["fuzzed"]) == 3000, line
        assert 1 <= int(f["valid"]) <= 3                                   # (the packet, and "another width / height")
        assert 0 < int(f["fuzzed_valid"]) < 3000, line                     # (the fuzz reaches both outcomes)


# ---- 5. the ABI -----------------------------------------------------------------------------------------------------------------------
def test_struct_mirrors_match_the_header():
    fields = [("fovpt_packet_pass", abi.PacketPass, [n for n, _ in abi.PacketPass._fields_], {}),
              ("fovpt_packet_header", abi.PacketHeader, [n for n, _ in abi.PacketHeader._fields_], {"passes": "pass"})]
    lines, consts = header_layout.probe([(cname, names, ren) for cname, _, names, ren in fields],
                                        ("FOVPT_PACKET_MAGIC", "FOVPT_PACKET_VERSION", "FOVPT_PACKET_SLOTS", "FOVPT_PACKET_NEAREST", "FOVPT_PACKET_SMOOTH"))
    for (cname, T, names, _), got in zip(fields, lines):
        assert got[0] == C.sizeof(T) == {"fovpt_packet_pass": 32, "fovpt_packet_header": 128}[cname]
        assert got[1:] == [getattr(T, n).offset for n in names]
    assert consts == [abi.PACKET_MAGIC, abi.PACKET_VERSION, abi.PACKET_SLOTS, abi.PACKET_NEAREST, abi.PACKET_SMOOTH]
    assert (pk.MAGIC, pk.VERSION, pk.SLOTS, pk.NEAREST, pk.SMOOTH) == (abi.PACKET_MAGIC, abi.PACKET_VERSION, abi.PACKET_SLOTS, abi.PACKET_NEAREST, abi.PACKET_SMOOTH)


def test_prototypes_symbols_and_the_shim(libs):
    text = open(os.path.join(ROOT, "include", "fovpt.h")).read()
    names = ["fovpt_packet_describe", "fovpt_packet_encode", "fovpt_packet_submit", "fovpt_packet_wait", "fovpt_packet_decode",
             "fovpt_packet_check", "fovpt_packet_decode_host"]
    full = dict(libs)["libfovpt.so"]
    for n in names:
        assert ("int %s(" % n) in text and n in lib.EXPORTS and hasattr(full, n), n
    loader = C.CDLL(lib.LOADER_SO_PATH)
    for n in lib.PACKET_HOST_EXPORTS:
        assert hasattr(loader, n), n
    assert not hasattr(loader, "fovpt_packet_encode")                     # (the context's entry points need the device)
    deps = subprocess.run(["ldd", lib.LOADER_SO_PATH], capture_output=True, text=True).stdout
    assert "hip" not in deps.lower() and "hsa" not in deps.lower() and "rocm" not in deps.lower(), deps
    shim = open(os.path.join(ROOT, "include", "SimplePathtracer.h")).read()
    for n in ("submitPacket", "waitPacket", "decodePacket"):
        assert n in shim, n
    header_layout.syntax_check_file(os.path.join(ROOT, "tests", "cpp", "shim_compile_check.cpp"))
    # the context's entry points without a context
    assert full.fovpt_packet_describe(None, None, 0, None) == E_INVALID and full.fovpt_packet_encode(None, None, None, 0, None) == E_INVALID
    assert full.fovpt_packet_submit(None, None, None, 0, None) == E_INVALID and full.fovpt_packet_wait(None, 0, None, None) == E_INVALID
    assert full.fovpt_packet_decode(None, None, None, 0, None) == E_INVALID


def test_a_client_decodes_with_the_loader_library_alone(tmp_path):
    """A fresh interpreter that only decodes a packet maps libfovpt_loader.so and neither libfovpt.so nor the HIP runtime."""
    size, gaze, radii, uniform = SHAPES[1]
    img = random_frame(size, 8)
    packet = pk.encode(img, size, gaze, radii, uniform)
    (tmp_path / "p.bin").write_bytes(packet)
    want = pk.decode(packet, pk.SMOOTH, np.zeros((size[1], size[0]), np.uint32))
    want.tofile(str(tmp_path / "want.bin"))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from fovpathtracing_optixcodelatest_amd import renderer\n"
            "got = renderer.decode_packet(open(%r, 'rb').read(), 1)\n"
            "assert got.shape == (%d, %d) and np.array_equal(got, np.fromfile(%r, np.uint32).reshape(got.shape))\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libfovpt_loader.so' in maps and 'libfovpt.so' not in maps and 'libamdhip64' not in maps, maps[-2000:]\n"
            % (ROOT, str(tmp_path / "p.bin"), size[1], size[0], str(tmp_path / "want.bin")))
    env = {k: v for k, v in os.environ.items() if k != "FOVPT_SO"}
    res = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
