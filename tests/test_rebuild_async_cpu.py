"""FOVPT_UPDATE_REBUILD_ASYNC without a GPU: the header, abi.py and the C++ shim agree on the new constants and on
fovpt_rebuild_info; the library exports fovpt_rebuild_state and links the thread library; and the state machine of the background
rebuild (csrc/fovpt_bgjob.h), driven by a fake build in tests/cpp/bgjob_test.cpp, holds under the thread sanitizer and under the
address and undefined-behaviour sanitizers (a stand-alone program: no HIP, no preloaded runtime)."""
import ctypes as C
import os
import subprocess

import pytest

import header_layout
from fovpathtracing_optixcodelatest_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "fovpathtracing_optixcodelatest_amd", "csrc")
CONSTANTS = (("FOVPT_UPDATE_REBUILD_ASYNC", "UPDATE_REBUILD_ASYNC"), ("FOVPT_REBUILD_IDLE", "REBUILD_IDLE"),
             ("FOVPT_REBUILD_BUILDING", "REBUILD_BUILDING"), ("FOVPT_REBUILD_READY", "REBUILD_READY"),
             ("FOVPT_REBUILD_WAIT", "REBUILD_WAIT"), ("FOVPT_REBUILD_ADOPT", "REBUILD_ADOPT"))


def test_constants_and_rebuild_info_mirror_the_header():
    """abi.py's constants are the header's, and abi.RebuildInfo is fovpt_rebuild_info member for member (the header compiled by
    gcc says where each member lies)."""
    names = [f[0] for f in abi.RebuildInfo._fields_]
    (got,), consts = header_layout.probe([("fovpt_rebuild_info", abi.RebuildInfo)], [c for c, _ in CONSTANTS])
    assert consts == [getattr(abi, a) for _, a in CONSTANTS]
    assert got[0] == C.sizeof(abi.RebuildInfo) == 64
    assert got[1:] == [getattr(abi.RebuildInfo, n).offset for n in names]
    assert names == ["state", "last_error", "requested", "started", "adopted", "failed", "discarded", "snapshot_update", "ms_build"]
    # the flag is a bit of its own beside the two the update calls had, and the bits they refused before stay refused
    assert abi.UPDATE_REBUILD_ASYNC & (abi.UPDATE_DEVICE | abi.UPDATE_REBUILD | 4 | 8) == 0
    assert bin(abi.UPDATE_REBUILD_ASYNC).count("1") == 1


def test_the_cpp_shim_maps_its_third_choice_to_the_flag():
    """include/SimplePathtracer.h: false / true / REBUILD_ASYNC of the updateAccel family are 0 / FOVPT_UPDATE_REBUILD /
    FOVPT_UPDATE_REBUILD_ASYNC, and rebuildState returns the C struct."""
    src = ('#include "SimplePathtracer.h"\n'
           "static_assert(SampleRenderer::rebuildFlag(false) == 0, \"\");\n"
           "static_assert(SampleRenderer::rebuildFlag(true) == FOVPT_UPDATE_REBUILD, \"\");\n"
           "static_assert(SampleRenderer::rebuildFlag(SampleRenderer::REBUILD) == FOVPT_UPDATE_REBUILD, \"\");\n"
           "static_assert(SampleRenderer::rebuildFlag(SampleRenderer::REBUILD_ASYNC) == FOVPT_UPDATE_REBUILD_ASYNC, \"\");\n"
           "static_assert(FOVPT_UPDATE_REBUILD_ASYNC == %d && sizeof(fovpt_rebuild_info) == %d, \"\");\n"
           "fovpt_rebuild_info (SampleRenderer::*state)(bool, bool) = &SampleRenderer::rebuildState;\n"
           "void (SampleRenderer::*accel)(const std::vector<int>&, int) = &SampleRenderer::updateAccel;\n"
           "void (SampleRenderer::*anim)(int, float, int) = &SampleRenderer::updateAnimated;\n"
           "int main() { return 0; }\n" % (abi.UPDATE_REBUILD_ASYNC, C.sizeof(abi.RebuildInfo)))
    header_layout.syntax_check(src)


def test_library_exports_rebuild_state_and_links_threads():
    lib.build()
    L = lib.load()
    assert hasattr(L, "fovpt_rebuild_state") and "fovpt_rebuild_state" in lib.EXPORTS
    out = abi.RebuildInfo()
    assert L.fovpt_rebuild_state(None, 0, C.byref(out)) == -1            # FOVPT_E_INVALID: null ctx
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert any("-shared" in line and "-pthread" in line and "$(OBJS)" in line for line in makefile.splitlines())


def test_no_kernel_file_includes_the_job_header():
    """csrc/fovpt_bgjob.h is host only and knows nothing of HIP: that is what lets the state machine run without a device."""
    text = open(os.path.join(CSRC, "fovpt_bgjob.h")).read()
    assert "#include <hip" not in text and "hipStream" not in text and "hipEvent" not in text and "fovpt_device.h" not in text
    for f in os.listdir(CSRC):
        if f.endswith(".hip") and not f.startswith(("api_", "fovpt_api")):
            assert "fovpt_bgjob.h" not in open(os.path.join(CSRC, f)).read() and "fovpt_ctx.h" not in open(os.path.join(CSRC, f)).read(), f


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_state_machine_under_sanitizers(tmp_path, sanitizer):
    """request / finished / adopt; requests while BUILDING and while READY ignored and counted; failed, then a new request;
    discard-and-join while the fake build runs; destruction while it runs; 400 rounds with random delays.  Exit status 0 and no
    sanitizer report."""
    exe = str(tmp_path / ("bgjob_" + sanitizer.split(",")[0]))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all", "-pthread", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "bgjob_test.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "bgjob ok" in res.stdout
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
