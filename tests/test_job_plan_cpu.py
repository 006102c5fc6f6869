"""The frame engine's decisions (csrc/fovpt_jobplan.h: plan_job, pass_table, chunk_rows, shard_capacity) without a GPU.  The header
is compiled into the stand-alone program of tests/cpp/job_plan_test.cpp under the address and undefined-behaviour sanitizers
(nothing preloaded), fed the product of the input sets below, and every field of every plan is compared with the restatement
of tests/job_plan_ref.py, which was written from run_job and run_passes as they stood before the header existed.  Apart from the
restatement, every plan is held to the invariants the launches rely on."""
import os
import subprocess

import numpy as np
import pytest

import job_plan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fovpathtracing_optixcodelatest_amd", "csrc")

SLOTS = (1, 255, 256, 16383, 16384, 16385, 16640, ref.SETS_SLOT_LIMIT, ref.SETS_SLOT_LIMIT + 1, 2 ** 31 - 1)
AXES = (("lanes", (1, 2, 4)), ("nsets", (2, 3, 4, 8)), ("frames_in_flight", (0, 1, 2, 4)), ("chains_per_frame", (0, 1, 2)),
        ("chains_default", (1, 2)), ("world", (1, 2)), ("spread_occlusion", (0, 1, 2, 3, -1)), ("max_depth", (1, 2, 4, 5, 8, 32)),
        ("any_catcher", (0, 1)), ("chunked", (0, 1)))
JOBS_LAST_SET = ((0, 0), (1, 0), (2, 1), (5, 3), (7, 7))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("job_plan") / "job_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "job_plan_test.cpp"), "-o", exe])

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
        return res.stdout
    return run


def test_the_header_is_plain_cpp_and_defines_the_constants_once(driver):
    """<stdint.h> only and no HIP, so that g++ compiles it alone; the engine's constants have one definition each, here, with the
    values the restatement assumes."""
    text = open(os.path.join(CSRC, "fovpt_jobplan.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<stdint.h>"]
    assert not any(word in text for word in ("hipStream", "hipEvent", "hipError", "__global__", "__device__", "__host__"))
    assert "std::vector" not in text and "std::function" not in text and "malloc" not in text and "new " not in text
    names = ("FOVPT_BLOCK", "FOVPT_SHARDS", "FOVPT_MAX_ITERS", "FOVPT_MAX_PASSES", "FOVPT_NSQ", "FOVPT_MAX_LANES", "FOVPT_LANES_DEFAULT",
             "FOVPT_SETS_SLOT_LIMIT")
    sources = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".cpp"))}
    for name in names:
        where = [f for f, s in sources.items() if "#define %s " % name in s]
        assert where == ["fovpt_jobplan.h"], (name, where)
    got = [int(x) for x in driver("consts\n").split()]
    assert got == [ref.BLOCK, ref.SHARDS, ref.MAX_ITERS, ref.MAX_PASSES, ref.NSQ, ref.MAX_LANES, ref.LANES_DEFAULT, ref.SETS_SLOT_LIMIT]


def _grid_text(slots):
    lists = [(slots,)] + [v for _, v in AXES]
    text = "plans " + " ".join("%d %s" % (len(v), " ".join(str(x) for x in v)) for v in lists)
    return text + " %d %s\n" % (len(JOBS_LAST_SET), " ".join("%d %d" % p for p in JOBS_LAST_SET))


def _grid_inputs(slots):
    """The product of the input sets for one slot count, the last set varying fastest: as the driver walks it."""
    pairs = np.array(JOBS_LAST_SET, np.int64)
    mesh = np.meshgrid(*([np.array(v, np.int64) for _, v in AXES] + [np.arange(len(pairs))]), indexing="ij")
    kw = {name: m.ravel() for (name, _), m in zip(AXES, mesh)}
    kw["jobs"], kw["last_set"] = pairs[mesh[-1].ravel(), 0], pairs[mesh[-1].ravel(), 1]
    kw["slots"] = np.full(mesh[0].size, slots, np.int64)
    return kw


@pytest.mark.parametrize("slots", SLOTS)
def test_every_plan_of_the_grid_is_the_restatements_and_keeps_the_invariants(driver, slots):
    kw = _grid_inputs(slots)
    n = kw["slots"].size
    got = np.fromstring(driver(_grid_text(slots)), dtype=np.int64, sep=" ").reshape(n, len(ref.FIELDS))
    want = ref.plan(**kw)
    for k, name in enumerate(ref.FIELDS):
        bad = np.flatnonzero(got[:, k] != want[name])
        assert bad.size == 0, (name, {key: int(v[bad[0]]) for key, v in kw.items()}, int(got[bad[0], k]), int(want[name][bad[0]]))
    # the invariants, on what the header answered
    g = {name: got[:, k] for k, name in enumerate(ref.FIELDS)}
    two = g["two_chains"] == 1
    assert np.all((g["set_index"] < g["nrot"]) & (g["nrot"] <= 2 * ref.MAX_LANES))
    assert np.all((g["lane"] < g["lanes"]) & (g["lanes"] >= 1))
    assert np.all(kw["lanes"][two] >= 2) and np.all(g["nchains"] == np.where(two, 2, 1))
    assert np.all(g["slot_begin0"][two] == 0) and np.all(g["slot_end0"][two] == g["slot_begin1"][two]) and np.all(g["slot_end1"][two] == slots)
    assert np.all(g["slot_end0"][two] % ref.BLOCK == 0) and np.all(g["sel0"][two] == 1) and np.all(g["sel1"][two] == 2)
    assert np.all(g["lane0"][two] == 0) and np.all(g["lane1"][two] == 1)
    assert np.all((g["sel0"][~two] == 0) & (g["slot_begin0"][~two] == 0) & (g["slot_end0"][~two] == slots) & (g["lane0"][~two] == g["lane"][~two]))
    assert np.all((1 <= g["nsq"]) & (g["nsq"] <= np.minimum(g["iters"], ref.NSQ)))
    assert np.all(g["iters"] <= ref.MAX_ITERS)
    assert np.all((g["spread_it"] == -1) | ((g["spread_it"] >= 0) & (g["spread_it"] < g["iters"])))
    deep = g["iters"] > g["nsq"]
    assert np.all((g["spread_it"][deep] == -1) | (g["spread_it"][deep] == 1))
    # (the moved launch runs on lane 1's shadow stream: a context with one lane never moves one)
    assert np.all(kw["lanes"][g["spread_it"] >= 0] >= 2)


def test_the_grid_reaches_every_branch(driver):
    """Both answers of every decision occur in the product, so that the comparison above is one of all of them."""
    seen = {name: set() for name in ("nrot", "lane", "two_chains", "nsq", "spread_kind")}
    for slots in (16384, ref.SETS_SLOT_LIMIT + 1):
        kw = _grid_inputs(slots)
        w = ref.plan(**kw)
        for name in ("nrot", "lane", "two_chains", "nsq"):
            seen[name] |= set(np.unique(w[name]).tolist())
        seen["spread_kind"] |= set(np.unique(np.where(w["spread_it"] < 0, -1, np.where(w["spread_it"] == w["iters"] - 1, 2, 1))).tolist())
    assert seen["nrot"] >= {2, 3, 4, 8} and seen["lane"] >= {0, 1, 3} and seen["two_chains"] == {0, 1} and seen["nsq"] == {1, 2, 4}
    assert seen["spread_kind"] == {-1, 1, 2}          # none, the second, the last


@pytest.mark.parametrize("slots", SLOTS)
def test_shard_capacity(driver, slots):
    cap = int(driver("cap %d\n" % slots))
    assert cap == ref.shard_capacity(slots)
    assert cap * ref.SHARDS >= slots + 512 * ref.SHARDS - 7


def test_grids_are_rounded_up_to_the_shards(driver):
    blocks = (1, 7, 8, 9, 1024, 2047, 2048, 6144, 256 * 24 + 3)
    got = [int(x) for x in driver("".join("grid %d\n" % b for b in blocks)).split()]
    assert got == [(b + ref.SHARDS - 1) // ref.SHARDS * ref.SHARDS for b in blocks]


# ---- the pass table and the chunks of an over-budget launch ----------------------------------------------------------------------
FRAME = ref.foveated_passes(96, 64, 12, 28, (1, 2, 8))        # the 96 x 64 frame of tests/test_streams_gpu.py


def _chunks(driver, budget, p, gw, gh, spp):
    lines = driver("chunks %d %d %d %d %d\n" % (budget, p, gw, gh, spp)).splitlines()
    assert lines[-1] == "end" and lines[0].split()[0] == "rows"
    return int(lines[0].split()[1]), int(lines[0].split()[3]), [tuple(int(x) for x in line.split()) for line in lines[1:-1]]


def test_whole_frame_pass_table(driver):
    text = "passes 0 0 0 %d %s\n" % (len(FRAME), " ".join("%d %d %d" % p for p in FRAME))
    lines = driver(text).splitlines()
    table, slots = ref.whole_frame(FRAME)
    assert lines[0] == "slots %d" % slots and slots == 24 * 16 * 1 + 30 * 30 * 2 + 26 * 26 * 8
    assert [tuple(int(x) for x in line.split()) for line in lines[1:]] == table


@pytest.mark.parametrize("budget", [3000, 700])
def test_chunks_tile_every_pass_in_ascending_rows_within_the_budget(driver, budget):
    assert ref.whole_frame(FRAME)[1] > budget
    ragged = 0
    for p, (gw, gh, spp) in enumerate(FRAME):
        rows, per_row, jobs = _chunks(driver, budget, p, gw, gh, spp)
        assert jobs == ref.chunk_jobs(budget, p, gw, gh, spp) and per_row == gw * spp and rows == budget // per_row
        assert jobs[0][0] == 0 and jobs[-1][1] == gh
        assert all(a[1] == b[0] for a, b in zip(jobs, jobs[1:])) and all(r0 < r1 for r0, r1, _, _ in jobs)
        assert all(fp == p and s == gw * (r1 - r0) * spp and 0 < s <= budget for r0, r1, fp, s in jobs)
        ragged += gh % rows != 0 and len(jobs) > 1
    assert budget != 700 or ragged >= 2            # gh no multiple of the rows per chunk: the last chunk is shorter


def test_a_row_above_the_budget_is_refused_with_the_engines_text(driver):
    gw, gh, spp = FRAME[2]
    rows, per_row, jobs = _chunks(driver, 207, 2, gw, gh, spp)
    assert (rows, per_row, jobs) == (0, 208, [])
    with pytest.raises(ref.PlanError, match="one launch row needs 208 sample slots \\(budget 207\\)"):
        ref.chunk_jobs(207, 2, gw, gh, spp)
    assert _chunks(driver, 208, 2, gw, gh, spp)[0] == 1          # one row exactly: chunks of one row
    api = open(os.path.join(CSRC, "fovpt_api.hip")).read()
    assert '"one launch row needs %llu sample slots (budget %llu)", (unsigned long long)cr.per_row, (unsigned long long)budget' in api


def test_a_pass_without_samples_is_refused(driver):
    assert driver("passes 0 0 0 2 24 16 1 30 30 0\n").strip() == "fail"
    with pytest.raises(ref.PlanError, match=ref.SPP_TEXT):
        ref.whole_frame([(24, 16, 1), (30, 30, 0)])
    api = open(os.path.join(CSRC, "fovpt_api.hip")).read()
    assert api.count('"' + ref.SPP_TEXT) == 1 and api.count("pass_table(") == 1       # one builder, one text


def test_a_chunk_keeps_its_place_in_the_frame(driver):
    """A chunk job holds one pass, rows [row0, row1), and the pass's index in the caller's frame."""
    lines = driver("passes 11 22 1 1 30 30 2\n").splitlines()
    assert lines == ["slots %d" % (30 * 11 * 2), "30 30 2 11 22 1"]
