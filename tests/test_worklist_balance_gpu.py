"""The rollout kernel's work lists against bytes recorded from the build before they were balanced
(tests/golden/rollout_worklists.npz, written by tools/make_worklist_golden.py from the library ROVMPC_LIB names).

Beside the theta chain the other waves of a workgroup take the per-node geometry: every item through phase 4a, the first
`early` items also through phase 4b.  Which lane evaluates an item does not enter its arithmetic, so however the items are
dealt out to the waves, J[K] (rovmpc_rollout_costs, rovmpc_batch_costs_device) and the step's record are the same bytes.
The cases of worklist_cases.py are the smallest at which the partition can go wrong: 40 candidates (two full workgroups
and one with 8 valid candidates), workgroups of 192 to 512 threads around the early batch (64 items, 16 items, none, with
two rounds left after the join), single precision, the hiprtc route and the theta loop with run-time flags; each with the
horizon as a literal of the kernel instance and as a run-time value."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_controller_helpers import rv  # noqa: E402,F401
from plan_golden_cases import load_fixture  # noqa: E402
from worklist_cases import CASES, LITERAL, run_case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_fixture(os.path.join(golden_dir, "rollout_worklists.npz"))


def test_fixture_names_its_origin(golden):
    assert len(str(golden["meta/parent_commit"])) == 40
    assert "gfx950" in str(golden["meta/version"]) and str(golden["meta/gfx"]).startswith("gfx950")
    assert {k.split("/")[0] for k in golden} - {"meta"} == {c.name for c in CASES}


@pytest.mark.parametrize("tag,no_literal_n", LITERAL, ids=[t for t, _ in LITERAL])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_bytes_of_the_recorded_build(rv, golden, case, tag, no_literal_n):
    got = run_case(rv, case, no_literal_n)
    prefix = f"{case.name}/{tag}/"
    want = {k[len(prefix):]: v for k, v in golden.items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want)
    for part, a in got.items():
        b = want[part]
        assert a.shape == b.shape and a.dtype == b.dtype, (part, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (part, np.argwhere(a != b)[:4])
