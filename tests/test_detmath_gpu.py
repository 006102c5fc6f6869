"""include/fovpt_detmath.h on gfx950 (fovpt_debug_math, one launch per op) over each function's whole stated domain:

  * the device's bits equal the host's (oracle.math_op) on every case set of detmath_cases.py, NaN by class
  * the device within detmath_ref.BOUND_ULP = 0.5 + 2**-20 binary32 ulp of the float64 reference directly (sqrt and divide:
    equal to numpy's correctly rounded float32 results), specials exact
  * the device reproduces tests/golden/detmath_frozen.json, the output bits an earlier revision's header gave on the
    production-domain inputs
"""
import json
import os

import numpy as np
import pytest

from fovpathtracing_optixcodelatest_amd import abi, scenes

import detmath_cases as dc
import detmath_ref as ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDS = [dc.NAMES[op] for op in dc.ALL_OPS]


@pytest.fixture(scope="module")
def device_results():
    """op -> the device's results on the op's case set; one renderer, one debug_math call per op."""
    from fovpathtracing_optixcodelatest_amd import renderer
    r = renderer.SampleRenderer(scenes.cornell_box())
    out = {}
    for op in dc.ALL_OPS:
        c = dc.cases(op)
        out[op] = r.debug_math(op, c.a, c.b)
    r.close()
    return out


@pytest.mark.parametrize("op", dc.ALL_OPS, ids=IDS)
def test_device_bits_equal_host_bits(oracle, device_results, op):
    c = dc.cases(op)
    want = oracle.math_op(op, c.a, c.b)
    bad = ~ref.same_bits(device_results[op], want)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail("%s: %d of %d results differ from the host's, first at a=%s b=%s: device %s, host %s" % (
            dc.NAMES[op], bad.sum(), bad.size, float(c.a[i]).hex(), float(c.b[i]).hex() if c.b is not None else None,
            float(device_results[op][i]).hex(), float(want[i]).hex()))


@pytest.mark.parametrize("op", dc.ALL_OPS, ids=IDS)
def test_device_within_bound_over_the_domain(device_results, op):
    c = dc.cases(op)
    got = device_results[op]
    if op in (abi.OP_SQRT, abi.OP_DIV):
        with np.errstate(all="ignore"):
            want = np.sqrt(c.a) if op == abi.OP_SQRT else np.divide(c.a, c.b)
        bad = ~ref.same_bits(got, want)
        assert not bad.any(), "%s: %d results differ from the correctly rounded one, first at %d" % (dc.NAMES[op], bad.sum(), np.flatnonzero(bad)[0])
        return
    err = ref.ulp_error(got, ref.exact(op, c.a, c.b))
    print("%s: device max error %s over %d inputs" % (dc.NAMES[op], ref.worst(err, c.a, c.b), c.a.size))
    assert (err <= ref.BOUND_ULP).all(), "%s: %s" % (dc.NAMES[op], ref.worst(err, c.a, c.b))


@pytest.mark.parametrize("op", dc.FROZEN_OPS, ids=[dc.NAMES[op] for op in dc.FROZEN_OPS])
def test_device_reproduces_frozen_bits(device_results, op):
    with open(os.path.join(GOLD, "detmath_frozen.json")) as f:
        want = json.load(f)["ops"][dc.NAMES[op]]
    assert int(dc.cases(op).frozen.sum()) == want["inputs"]
    assert dc.frozen_digest(op, device_results[op]) == want["sha256"], "%s: a production-domain result moved" % dc.NAMES[op]
