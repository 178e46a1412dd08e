"""The rollout kernel's prologue against bytes recorded from the build before its loads and set-up were moved
(tests/golden/rollout_prologue.npz, written by tools/make_prologue_golden.py from the library ROVMPC_LIB names).

Phase 0 copies the workgroup's candidate controls into LDS; the gamma wave and the theta wave then prepare their chains'
constants and start values.  When a load is issued, and on which side of a barrier a value is formed that does not depend
on that barrier, enters no result's arithmetic: J[K], every trajectory and the step's record are the same bytes.  The cases
of prologue_cases.py are the smallest at which that can go wrong:
  * control copy: 19 and 40 candidates (a last workgroup with 3 and with 8 valid ones), horizons 1, 7 (21-element rows: the
    16-byte chunks straddle candidates) and 20, both precisions, workgroups of 64 to 512 threads; the candidate tensor
    compact, as a view one element into a larger buffer (the unaligned path) and between NaN neighbours; three problems in
    one launch; the sampled step;
  * set-up: theta_0 of 0.6 and 1.5, beyond 2^26 (the out-of-line reduction) and NaN, Euler and HOLD (the theta loop with
    run-time flags), the three velocity-transform modes, the horizon as a literal and as a run-time value;
  * fifty steps of the pipelined closed loop with feedback (theta_0 arrives through the ring)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_controller_helpers import rv  # noqa: E402,F401
from plan_golden_cases import load_fixture  # noqa: E402
import prologue_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_fixture(os.path.join(golden_dir, "rollout_prologue.npz"))


def assert_same_bytes(got, golden, prefix):
    want = {k[len(prefix):]: v for k, v in golden.items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want)
    for part, a in got.items():
        b = want[part]
        a = np.asarray(a)
        assert a.shape == b.shape and a.dtype == b.dtype, (part, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (part, np.argwhere(a.view(np.uint8) != b.view(np.uint8))[:4])


def test_fixture_names_its_origin(golden):
    assert len(str(golden["meta/parent_commit"])) == 40
    assert "gfx950" in str(golden["meta/version"]) and str(golden["meta/gfx"]).startswith("gfx950")
    assert {k.rsplit("/", 2)[0] if k.startswith("copy/") else k.split("/")[0] for k in golden} - {"meta"} == \
        {f"copy/{c.name}" for c in pc.COPY_CASES} | {"batch3", "sampled", "setup", "loop"}


def layouts_agree(got):
    """Every part of the unaligned and of the NaN-fenced view equals the compact run's."""
    for k, a in got.items():
        layout, part = k.split("/", 1)
        assert a.tobytes() == got[f"compact/{part}"].tobytes(), k


@pytest.mark.parametrize("case", pc.COPY_CASES, ids=[c.name for c in pc.COPY_CASES])
def test_control_copy(rv, golden, case):
    got = pc.run_copy_case(rv, case)
    layouts_agree(got)
    for layout in pc.LAYOUTS:
        assert np.isfinite(got[f"{layout}/batch_J"]).all() and np.isfinite(got[f"{layout}/step_record"]).all()
    assert_same_bytes(got, golden, f"copy/{case.name}/")


def test_three_problems_in_one_launch(rv, golden):
    got = pc.run_batch_case(rv)
    layouts_agree(got)
    assert np.isfinite(got["fenced/batch_J"]).all()
    assert_same_bytes(got, golden, "batch3/")


def test_sampled_step(rv, golden):
    assert_same_bytes(pc.run_sampled_case(rv), golden, "sampled/")


@pytest.mark.parametrize("tag,no_literal_n", pc.LITERAL, ids=[t for t, _ in pc.LITERAL])
@pytest.mark.parametrize("case", pc.SETUP_CASES, ids=[c.name for c in pc.SETUP_CASES])
def test_hoisted_setup(rv, golden, case, tag, no_literal_n):
    got = pc.run_setup_case(rv, case, no_literal_n)
    if np.isnan(case.theta0):
        # theta is NaN from node 0 on, gamma's path does not read it; every cost is NaN, reported as +inf
        assert np.isnan(got["traj"][:, :, 0]).all() and np.isfinite(got["traj"][:, :, 1]).all()
        assert got["step_record"][0] == np.inf and got["step_record"][1] == 0.0
    else:
        assert np.isfinite(got["costs_J"]).all() and np.isfinite(got["traj"]).all()
    assert_same_bytes(got, golden, f"setup/{case.name}/{tag}/")


def test_pipelined_closed_loop(rv, golden):
    got = pc.run_loop_case(rv)
    assert np.isfinite(got["records"]).all()
    assert_same_bytes(got, golden, "loop/")
