"""The post-processing fuzz's seed-to-parameters generator (tests/postprocess_fuzz.py) without a GPU: the default seed range
reaches every edge the GPU fuzz (tests/test_postprocess_fuzz_gpu.py) is there to cover."""
import math

import postprocess_fuzz as pf
from fovpathtracing_optixcodelatest_amd import abi


def test_the_default_seeds_cover_every_edge():
    ps = [pf.params(s) for s in pf.DEFAULT_SEEDS]
    assert [p["size"] for p in ps[:len(pf.EDGE_SHAPES)]] == pf.EDGE_SHAPES
    assert all(1 <= p["size"][0] <= 200 and 1 <= p["size"][1] <= 130 for p in ps)
    assert any(not (0 <= p["gaze"][0] < p["size"][0] and 0 <= p["gaze"][1] < p["size"][1]) for p in ps)
    assert any(p["gaze"][0] < 0 for p in ps) and any(p["gaze"][1] < 0 for p in ps)
    assert any(p["radii"] == (0, 0) for p in ps)
    assert any(p["radii"][0] == p["radii"][1] > 0 for p in ps)
    assert any(p["radii"][1] > math.hypot(*p["size"]) for p in ps if not p["uniform"])
    for flag in ("uniform", "accumulate"):
        assert {p[flag] for p in ps} == {0, 1}, flag
    assert {p["scene"] for p in ps} == set(pf.SCENES)
    den = [p["denoise"] for p in ps if p["denoise"] is not None]
    for lv in pf.LEVELS:
        assert {d[lv] for d in den} == set(range(abi.DENOISE_MAX_ITERATIONS + 1)), lv
    assert any(all(d[lv] == 0 for lv in pf.LEVELS) for d in den)
    assert any(all(d[lv] == abi.DENOISE_MAX_ITERATIONS for lv in pf.LEVELS) for d in den)
    rec = [p["reconstruct"] for p in ps]
    assert {r["levels"] for r in rec} == {0, 1, 2, 3}
    assert {r["remodulate"] for r in rec} == {0, 1}
    assert {r["support"] for r in rec} >= {1.0, 2.0} and any(1.0 < r["support"] < 2.0 for r in rec)
    assert any(p["reconstruct"]["remodulate"] == 0 and not p["write_guides"] for p in ps)
    assert {p["reconstruct_input"] for p in ps} == {"accum", "denoised"}
    assert {p["caller_buffers"] for p in ps} == {False, True}
    for k in pf.DENOISE_SIGMAS:
        assert {abi.SIGMA_MIN, abi.SIGMA_MAX} <= {d[k] for d in den}, k
    for k in pf.RECONSTRUCT_SIGMAS:
        assert {abi.SIGMA_MIN, abi.SIGMA_MAX} <= {r[k] for r in rec}, k
    for p in ps:                                         # every sigma inside the accepted range
        for d in (p["denoise"] or {}, p["reconstruct"]):
            for k, v in d.items():
                if k.endswith("_sigma"):
                    assert abi.SIGMA_MIN <= v <= abi.SIGMA_MAX, (p["seed"], k, v)
    for seed in range(0, 1000):                          # also a sweep's seeds: configs fovpt_set_config accepts
        r_inner, r_outer = pf.params(seed)["radii"]
        assert 0 <= r_inner <= r_outer, seed
    # the frames the main-path fuzz never renders (w < 17 or h < 9) are held against the oracle here
    assert sum(p["size"][0] < 17 or p["size"][1] < 9 for p in ps) >= len(pf.EDGE_SHAPES)
