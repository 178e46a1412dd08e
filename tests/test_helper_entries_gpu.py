"""The host-pointer helper entries (rovmpc_predict ... rovmpc_kabsch_velocity_transform, rovmpc_math_probe) against bits
recorded from an earlier build (tests/golden/helper_entries.npz), on the cases of helper_golden_cases.py: the smallest shapes
that use every upload and every copy back.

Per case: every output equals the recorded array byte for byte (NaN positions and payloads included); the same call with its
optional outputs null, one at a time and all together, gives the same bytes for the outputs that remain; the empty input,
where the entry allows one, returns ROVMPC_OK and leaves a poisoned output untouched; one bad argument is refused with
ROVMPC_ERR_INVALID and the entry's name in rovmpc_last_error.

The fixture is written by tools/make_helper_golden.py from the library ROVMPC_LIB names; a change to the host code must pass
against it as it is, a change to the helper kernels that legitimately moves bits records it again."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_controller_helpers import rv  # noqa: E402,F401
import helper_golden_cases as hg  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return hg.load_fixture(os.path.join(golden_dir, "helper_entries.npz"))


@pytest.fixture(scope="module")
def eng(rv):
    with hg.handle(rv) as e:
        yield e


@pytest.fixture(scope="module")
def case_table(rv):
    return {c.name: c for c in hg.cases(rv)}


NAMES = (["predict_theta", "predict_gamma", "eval_expression"] +
         [f"math_probe_{fn}_{dt}" for dt in ("f64", "f32") for fn in ("sqrt", "div", "sincos")] +
         ["lagrangian_rollout", "replay_rk4", "replay_double_euler", "solve_catenary", "rodrigues", "catenary_points",
          "compute_catenary_3d", "transform_catenary", "velocity_transform", "extract_features", "features_dd",
          "gaussian_filter1d", "kabsch"])


def test_fixture_names_its_origin(golden, case_table):
    assert len(str(golden["meta/parent_commit"])) == 40
    assert "gfx950" in str(golden["meta/version"]) and str(golden["meta/gfx"]).startswith("gfx950")
    assert sorted(case_table) == sorted(NAMES)
    assert {k.split("/")[0] for k in golden} - {"meta"} == set(NAMES)


def _same_bits(case, part, a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (case, part, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), (case, part, a, b)


@pytest.mark.parametrize("name", NAMES)
def test_bits_of_the_recorded_build(eng, golden, case_table, name):
    case = case_table[name]
    want = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}
    rc, got = hg.call(eng, case)
    assert rc == hg.OK, hg.last_error(eng)
    assert sorted(got) == sorted(want)
    for part, a in got.items():
        _same_bits(name, part, a, want[part])
    # optional outputs null, one at a time and all together: the remaining outputs keep their bits
    opt = hg.optional_outputs(case)
    for null in [(o,) for o in opt] + ([tuple(opt)] if len(opt) > 1 else []):
        rc, got = hg.call(eng, case, null=null)
        assert rc == hg.OK, (null, hg.last_error(eng))
        assert sorted(got) == sorted(set(want) - set(null))
        for part, a in got.items():
            _same_bits(name, part + " without " + ",".join(null), a, want[part])


@pytest.mark.parametrize("name", NAMES)
def test_empty_input_and_bad_argument(eng, case_table, name):
    case = case_table[name]
    if case.empty is not None:
        rc, got = hg.call(eng, case, replace=(case.empty, 0))
        assert rc == hg.OK, hg.last_error(eng)
        for part, a in got.items():
            assert a.tobytes() == bytes([hg.POISON]) * a.nbytes, (name, part, a)
    rc, got = hg.call(eng, case, replace=case.bad)
    assert rc == hg.ERR_INVALID, (rc, hg.last_error(eng))
    assert case.fn in hg.last_error(eng), hg.last_error(eng)
    for part, a in got.items():
        assert a.tobytes() == bytes([hg.POISON]) * a.nbytes, (name, part, a)
