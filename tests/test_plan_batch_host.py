"""Batched MPPI and CEM on the host side: the six entry points are declared in the header, exported by the built library and
bound with the declared argument types; BatchedMPPI / BatchedCEM reject bad shapes, sizes, seeds and parameters with
ValueError before any library call; plans broadcast to (B, N, 3); and the oracle leaves every cost of the anchor problem of
test_plan_batch_gpu.py finite.  No compute call into the library happens here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import rovmpc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_controller_helpers import defaults, oracle_J  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I32, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
SIGNATURES = {
    "rovmpc_mppi_reset_batch": [P, I32, P],
    "rovmpc_mppi_step_batch": [P, I32, P, P, U64, ctypes.POINTER(rovmpc.MPPIParams), P, P, P],
    "rovmpc_mppi_last_batch": [P, P, P],
    "rovmpc_cem_reset_batch": [P, I32, P],
    "rovmpc_cem_step_batch": [P, I32, P, P, U64, ctypes.POINTER(rovmpc.CEMParams), P, P, P, P, P],
    "rovmpc_cem_last_batch": [P, P, P],
}


def _header():
    return open(os.path.join(ROOT, "include", "rovmpc.h")).read()


def test_header_declares_the_batched_entry_points():
    hdr = _header()
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*?)\);", hdr, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(args), name          # as many parameters as the binding has
        assert name in rovmpc.exported_symbols(), name
    # the law is stated, and "batched" has left the two "Not provided" lists
    assert "bit for bit what rovmpc_mppi_step(states[b], seeds[b], step, p)" in hdr
    for m in re.finditer(r"Not provided:(.*?)\*/", hdr, re.S):
        assert "batched" not in m.group(1)


def test_symbols_resolve_with_the_declared_types():
    lib = rovmpc.load_library()
    raw = ctypes.CDLL(rovmpc.LIB_PATH)
    for name, args in SIGNATURES.items():
        assert getattr(raw, name)                                        # exported by the built library itself
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int, name
        assert list(fn.argtypes) == args, name


def test_classes_exported():
    assert rovmpc.BatchedMPPI is rovmpc.mpc.BatchedMPPI and rovmpc.BatchedCEM is rovmpc.mpc.BatchedCEM
    for name in ("mppi_reset_batch", "mppi_step_batch", "mppi_last_batch", "cem_reset_batch", "cem_step_batch", "cem_last_batch"):
        assert callable(getattr(rovmpc.Engine, name)), name


# ---- ValueError before any library call (no handle is created: these pass without a GPU) -------------------------------
class _NoEngine:
    def __init__(self, *a, **k):
        raise AssertionError("the library was reached")


@pytest.fixture
def no_engine(monkeypatch):
    monkeypatch.setattr(rovmpc.mpc, "Engine", _NoEngine)


MPPI_BAD = [dict(B=0), dict(B=1025), dict(B=2.5), dict(B=True), dict(B=3, seeds=[1, 2]), dict(B=3, seeds=[1, 2, 3, 4]),
            dict(B=2, nominal=np.zeros((3, 6, 3))), dict(B=2, nominal=np.zeros((5, 3))), dict(B=2, nominal=np.zeros(4)),
            dict(B=2, nominal=np.zeros((2, 6, 2))), dict(B=2, lam=0.0), dict(B=2, lam=float("nan")), dict(B=2, n_iter=0),
            dict(B=2, n_iter=65), dict(B=2, std=(1.0, -1.0, 1.0)), dict(B=2, std=(1.0, 1.0))]


@pytest.mark.parametrize("kw", MPPI_BAD)
def test_batched_mppi_rejects(no_engine, kw):
    with pytest.raises(ValueError):
        rovmpc.BatchedMPPI(N=6, K=32, **kw)


CEM_BAD = [dict(B=0), dict(B=1025), dict(B=3, seeds=[1]), dict(B=2, mean=np.zeros((3, 6, 3))), dict(B=2, mean=np.zeros((6, 2))),
           dict(B=2, n_elite=0), dict(B=2, n_elite=33), dict(B=2, n_elite=1.5), dict(B=2, alpha=1.0), dict(B=2, alpha=-0.1),
           dict(B=2, n_iter=0), dict(B=2, std=(1.0, float("nan"), 1.0)), dict(B=2, std_min=(0.0, -1.0, 0.0)),
           dict(B=2, lo=(0.0, 0.0, 0.0), hi=(1.0, -1.0, 1.0)), dict(B=2, lo=(float("nan"), 0.0, 0.0)), dict(B=2, reserved=1)]


@pytest.mark.parametrize("kw", CEM_BAD)
def test_batched_cem_rejects(no_engine, kw):
    with pytest.raises(ValueError):
        rovmpc.BatchedCEM(N=6, K=32, **kw)


def test_accepted_arguments_reach_the_library(no_engine):
    """The same constructor with good arguments goes on to create a handle (here: the stand-in that says so)."""
    with pytest.raises(AssertionError, match="the library was reached"):
        rovmpc.BatchedMPPI(N=6, K=32, B=2, seeds=[5, 6], nominal=np.zeros((2, 6, 3)))
    with pytest.raises(AssertionError, match="the library was reached"):
        rovmpc.BatchedCEM(N=6, K=32, B=1024, n_elite=32, mean=np.zeros(3))


def test_states_are_checked():
    from rovmpc.mpc import batch_states
    st = np.arange(32, dtype=np.float64).reshape(2, 16)
    assert np.array_equal(batch_states(st, 2), st)
    assert np.array_equal(batch_states([st[0], list(st[1])], 2), st)
    s = rovmpc.MPCState(P0=(0, 0, 0), P1=(1, 2, 3), V1=(4, 5, 6), A1=(0, 0, 0), theta=0.1, gamma=0.2)
    d = dict(P0=(0, 0, 0), P1=(1, 2, 3), V1=(4, 5, 6), A1=(0, 0, 0), theta=0.1, gamma=0.2)
    got = batch_states([s, d], 2)
    assert got.shape == (2, 16) and np.array_equal(got[0], got[1]) and np.array_equal(got[0], s.as_array())
    for bad in (st[:1], np.zeros((2, 15)), [st[0]], np.zeros(16), []):
        with pytest.raises(ValueError):
            batch_states(bad, 2)


# ---- plans and seeds ---------------------------------------------------------------------------------------------------
def test_plan_broadcasting():
    from rovmpc.mpc import batch_plans
    B, N = 3, 4
    default = np.array([7.0, 8.0, 9.0])
    one, node, full = np.array([1.0, 2.0, 3.0]), np.arange(N * 3, dtype=np.float64).reshape(N, 3), \
        np.arange(B * N * 3, dtype=np.float64).reshape(B, N, 3)
    for value, want in ((None, np.tile(default, (B, N, 1))), (one, np.tile(one, (B, N, 1))), (node, np.tile(node, (B, 1, 1))),
                        (full, full)):
        got = batch_plans(value, B, N, default, "plan")
        assert got.shape == (B, N, 3) and got.dtype == np.float64 and got.flags.c_contiguous and got.flags.writeable
        assert np.array_equal(got, want)
    for bad in (np.zeros((B, N, 2)), np.zeros((B + 1, N, 3)), np.zeros((N + 1, 3)), np.zeros(2), np.zeros((1, N, 3))):
        with pytest.raises(ValueError):
            batch_plans(bad, B, N, default, "plan")


def test_default_seeds():
    from rovmpc.mpc import batch_seeds
    assert batch_seeds(None, 20250523, 4).tolist() == [20250523, 20250524, 20250525, 20250526]
    got = batch_seeds([3, 2 ** 64 - 1, 5], 0, 3)
    assert got.dtype == np.uint64 and got.tolist() == [3, 2 ** 64 - 1, 5]
    with pytest.raises(ValueError):
        batch_seeds([1, 2], 0, 3)


# ---- the anchor of test_plan_batch_gpu.py::test_c2_costs_against_the_oracle ------------------------------------------------
def test_oracle_leaves_every_cost_of_the_anchor_finite():
    """Problem B - 1 = 2 of the C2-sized batch: the synthetic state, the default nominal, seed + 2, counter 0."""
    from oracle import rovmpc_oracle as orc
    N, K = 20, 4096
    model = rovmpc.default_model()
    cfg = rovmpc.MPCConfig(N=N, K=K)
    nu, std = defaults(rovmpc, N)
    state, _ = rovmpc.synthetic_problem(K, N)
    z = orc.philox_normals(20250523 + 2, 0, K * N * 3).reshape(K, N, 3)     # the sampler's law: U[0] = nu, U[k] = nu + std z
    U = nu[None] + np.asarray(std, dtype=np.float64) * z
    U[0] = nu
    J, _ = oracle_J(orc, cfg, model, state, U)
    assert np.isfinite(J).all()
