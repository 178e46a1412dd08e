"""The MPPI and CEM controller entry points against bits recorded from an earlier build (tests/golden/plan_controllers.npz):
single steps, batched steps (B = 1 included), the device loops with the host step after them, rovmpc_*_update_device and a
batch with a problem that has no finite cost.  Every case of plan_golden_cases.py: records, plans, spreads, elite lists and
stats of every step, and the SHA-256 of the last candidates and costs.

test_plan_batch_gpu.py and test_plan_loop_gpu.py hold the batched entries to the single ones; both run through one host
path, so a mistake in it that both share (a wrong counter, half or row offset) shows only against recorded bits.

The fixture is written by tools/make_plan_golden.py from the library ROVMPC_LIB names; it names the commit, rovmpc_version()
and the gfx target it was taken on.  A change to the kernels that legitimately moves bits records it again with the same
tool; a change to the host code must pass against the fixture as it is.

Comparisons are exact: the arrays' bytes, and np.array_equal with NaN equal to NaN for the stats."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_controller_helpers import rv  # noqa: E402,F401
from plan_golden_cases import CASES, lam_key, load_fixture, run_case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_fixture(os.path.join(golden_dir, "plan_controllers.npz"))


def test_fixture_names_its_origin(golden):
    assert len(str(golden["meta/parent_commit"])) == 40
    assert "gfx950" in str(golden["meta/version"]) and str(golden["meta/gfx"]).startswith("gfx950")
    names = {k.split("/")[0] for k in golden} - {"meta", "lam"}
    assert names == {c.name for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_bits_of_the_recorded_build(rv, golden, case):
    got = run_case(rv, case, float(golden[lam_key(case)]))
    want = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(case.name + "/")}
    assert sorted(got) == sorted(want)
    for part, a in got.items():
        b = want[part]
        assert a.shape == b.shape and a.dtype == b.dtype, (part, a.shape, b.shape, a.dtype, b.dtype)
        if part.endswith("stats"):
            assert np.array_equal(a, b, equal_nan=True), (part, a, b)
        else:
            assert a.tobytes() == b.tobytes(), (part, np.argwhere(a != b)[:4])
