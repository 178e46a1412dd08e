"""The marker fit's entries against bits recorded from the build before its per-frame iteration moved into the device
function the tracker shares (tests/golden/fit_entries.npz, written by tools/make_fit_golden.py on the calls of
fit_golden_cases.py): every scene of fit_reference.scenes() from its own start and from each start of the tracker's default
list, by the host entry and by the device entry, byte for byte."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_reference as fr  # noqa: E402
import fit_golden_cases as fg  # noqa: E402
from plan_controller_helpers import rv  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "fit_entries.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_names_its_origin(golden):
    assert len(str(golden["meta_parent_commit"])) == 40
    assert "gfx950" in str(golden["meta_version"]) and str(golden["meta_gfx"]).startswith("gfx950")
    parts = sorted(k for k in golden if not k.startswith("meta_"))
    assert parts == sorted(["own"] + [f"start{k}" for k in range(len(fg.STARTS))])
    statuses = {fr.Status(int(s)) for k in parts for s in golden[k][:, 5]}
    assert statuses == set(fr.Status)
    assert all(golden[k].shape == (len(fr.scenes()), fr.OUT) for k in parts)


@pytest.mark.parametrize("device", (False, True), ids=("host-entry", "device-entry"))
def test_bits_of_the_recorded_build(rv, golden, device):
    got = fg.run(rv, device=device)
    for part, a in got.items():
        want = golden[part]
        bad = [fr.scenes()[i].name for i in range(len(a)) if a[i].tobytes() != want[i].tobytes()]
        assert not bad, (part, bad)
