"""The tether keep-out cost without a GPU: the values rovmpc.TetherCost accepts and refuses before any library call, the
type checks of tether= on the four controllers, and the ctypes mirror against include/rovmpc.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rovmpc
from rovmpc import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPH = [[0.1, 0.2, 0.3, 0.5], [1.0, -1.0, 0.0, 0.0]]


def _header():
    return open(os.path.join(ROOT, "include", "rovmpc.h")).read()


def test_header_declares_the_entry_points_and_the_law():
    hdr = _header()
    declared = set(re.findall(r"\b(rovmpc_[a-z_0-9]+)\s*\(", hdr))
    for name in ("rovmpc_set_tether_cost", "rovmpc_tether_cost_device"):
        assert name in declared and name in rovmpc.exported_symbols(), name
    assert re.search(r"typedef struct rovmpc_tether_cost \{.*?\} rovmpc_tether_cost;", hdr, re.S)
    for phrase in ("the chord", "build-defined", "beyond c_hi", "C_k = +inf", "applied first"):
        assert phrase in hdr, phrase


def test_struct_mirror_matches_the_header():
    body = re.search(r"typedef struct rovmpc_tether_cost \{(.*?)\} rovmpc_tether_cost;", _header(), re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+([a-z_]+)((?:\[[A-Z_0-9]+\])*)\s*;", body, re.M)
    assert [f[1] for f in fields] == [n for n, _ in _lib.TetherCost._fields_]
    n_max = int(re.search(r"#define ROVMPC_TETHER_MAX_SPHERES (\d+)", _header()).group(1))
    assert n_max == _lib.TETHER_MAX_SPHERES == 8
    size = sum({"int32_t": 4, "double": 8}[t] * (n_max * 4 if dims else 1) for t, _, dims in fields)
    assert C.sizeof(_lib.TetherCost) == size == 4 + 4 + 8 + 8 + 8 * 32
    t = _lib.tether_cost(SPH, 2.0, 0.25)
    assert t.struct_size == size and t.n_spheres == 2 and t.w == 2.0 and t.margin == 0.25
    assert list(t.spheres[1]) == SPH[1] and list(t.spheres[2]) == [0.0] * 4


def test_tether_cost_values():
    t = rovmpc.TetherCost(SPH, 3.0)
    assert t.w == 3.0 and t.margin == 0.0 and np.array_equal(t.spheres, np.array(SPH))
    assert rovmpc.TetherCost(SPH[0], 0.0, margin=0.5).spheres.shape == (1, 4)           # one sphere given flat; w = 0 allowed
    assert rovmpc.TetherCost(np.tile(SPH[0], (8, 1)), 1).spheres.shape == (8, 4)
    for bad in (dict(spheres=[], w=1.0), dict(spheres=np.tile(SPH[0], (9, 1)), w=1.0), dict(spheres=[[0, 0, 0]], w=1.0),
                dict(spheres=[[0, 0, 0, -1.0]], w=1.0), dict(spheres=[[0, np.nan, 0, 1.0]], w=1.0), dict(spheres=[[np.inf, 0, 0, 1.0]], w=1.0),
                dict(spheres=SPH, w=-1.0), dict(spheres=SPH, w=np.inf), dict(spheres=SPH, w=np.nan),
                dict(spheres=SPH, w=1.0, margin=-0.1), dict(spheres=SPH, w=1.0, margin=np.nan), dict(spheres=SPH, w=1.0, margin=np.inf)):
        with pytest.raises(ValueError):
            rovmpc.TetherCost(**bad)
    for bad in (dict(spheres=SPH, w="1"), dict(spheres=SPH, w=None), dict(spheres=SPH, w=[1.0]), dict(spheres=SPH, w=1.0, margin=(0.1,))):
        with pytest.raises(TypeError):
            rovmpc.TetherCost(**bad)


@pytest.mark.parametrize("ctl,kw", [(rovmpc.MPPI, {}), (rovmpc.CEM, {}), (rovmpc.BatchedMPPI, dict(B=2)), (rovmpc.BatchedCEM, dict(B=2))])
def test_tether_argument_is_type_checked_before_the_library(ctl, kw, monkeypatch):
    """A wrong tether= raises TypeError before an engine exists (the engine would need the GPU)."""
    from rovmpc import mpc

    def no_engine(*a, **k):
        raise AssertionError("the engine was created before the check")
    monkeypatch.setattr(mpc, "Engine", no_engine)
    for bad in ("sphere", 1.0, _lib.tether_cost(SPH, 1.0), [SPH]):
        with pytest.raises(TypeError):
            ctl(N=4, K=64, tether=bad, **kw)
    with pytest.raises(AssertionError):
        ctl(N=4, K=64, tether=rovmpc.TetherCost(SPH, 1.0), **kw)               # a good one reaches the engine
    with pytest.raises(TypeError):
        mpc.check_tether(object())
    assert mpc.check_tether(None) is None
