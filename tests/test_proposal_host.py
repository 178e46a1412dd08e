"""The shaped proposal of MPPI and CEM on the host side (rovmpc_set_noise_correlation, rovmpc_mppi_set_bounds): the header
declares the setters and the library exports them, the parameter structs keep their sizes, the Python layer checks beta and
the box before the library is called, and the NumPy restatement of the law (used by test_proposal_gpu.py) passes its own
checks.  No compute call into the library happens here."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

import rovmpc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cem_host import cem_clamp, cem_sample_ref  # noqa: E402
from test_mppi_host import mppi_sample_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTERS = ("rovmpc_set_noise_correlation", "rovmpc_mppi_set_bounds")
NO_BOX = ((-math.inf,) * 3, (math.inf,) * 3)

# the statistics case of the issue: seed 77, counter 0, K 4096, N 20
STAT_SEED, STAT_K, STAT_N, STAT_BETA, STAT_BOUND = 77, 4096, 20, (0.9, 0.5, 0.0), 0.05


# ---- the law of include/rovmpc.h (the shaped proposal), restated --------------------------------------------------------
def colored_noise(normals, seed, counter, K, N, beta):
    """eps (K, N, 3): eps[k][0] = z[k][0], eps[k][n] = beta eps[k][n-1] + sqrt((1 - beta)(1 + beta)) z[k][n], in float64;
    `normals` = oracle.philox_normals."""
    z = normals(seed, counter, K * N * 3).reshape(K, N, 3)
    beta = np.asarray(beta, dtype=np.float64)
    root = np.sqrt((1.0 - beta) * (1.0 + beta))
    eps = z.copy()
    for n in range(1, N):
        eps[:, n] = beta * eps[:, n - 1] + root * z[:, n]
    return eps


def proposal_sample_ref(normals, seed, counter, K, N, sigma, mean, beta, lo=NO_BOX[0], hi=NO_BOX[1], dtype=np.float64):
    """U[0] = (T) clamp(mean), U[k] = (T) clamp(mean + sigma eps[k]) for k >= 1; sigma (N, 3) or (3,).  MPPI: mean = nu,
    sigma = std, the handle's box; CEM: mean = mu, sigma = sigma_i, its parameters' box."""
    eps = colored_noise(normals, seed, counter, K, N, beta)
    mean = np.asarray(mean, dtype=np.float64)
    U = cem_clamp(mean[None] + np.asarray(sigma, dtype=np.float64) * eps, lo, hi).astype(dtype)
    U[0] = cem_clamp(mean, lo, hi).astype(dtype)
    return U


def lag_correlation(eps, lag):
    """Sample correlation per channel of eps[k][n] and eps[k][n + lag] over the candidates k >= 1 and all n."""
    a, b = eps[1:, :-lag].reshape(-1, 3), eps[1:, lag:].reshape(-1, 3)
    a, b = a - a.mean(axis=0), b - b.mean(axis=0)
    return (a * b).sum(axis=0) / np.sqrt((a * a).sum(axis=0) * (b * b).sum(axis=0))


def stat_inputs(rv):
    """(nominal (N, 3), std (3,)) of the statistics case, shared with test_proposal_gpu.py."""
    m = rv.default_model()
    nu = np.tile(m.mean[3:6], (STAT_N, 1)) + 0.01 * np.arange(STAT_N * 3).reshape(STAT_N, 3)
    return nu, np.asarray(m.scale[3:6], dtype=np.float64)


# ---- header, exports, bindings, struct sizes ----------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "rovmpc.h")) as f:
        return f.read()


def test_header_declares_the_setters_and_they_are_bound():
    hdr = _header()
    declared = set(re.findall(r"\b(rovmpc_[a-z_0-9]+)\s*\(", hdr))
    lib = rovmpc.load_library()
    for name in SETTERS:
        assert name in declared, name
        assert name in rovmpc.exported_symbols(), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert re.search(r"int rovmpc_set_noise_correlation\(rovmpc_handle \*h, const double \*beta3\);", hdr)
    assert re.search(r"int rovmpc_mppi_set_bounds\(rovmpc_handle \*h, const double \*lo3, const double \*hi3\);", hdr)
    assert len(lib.rovmpc_set_noise_correlation.argtypes) == 2 and len(lib.rovmpc_mppi_set_bounds.argtypes) == 3
    # "control bounds" is no longer listed as missing
    assert "control bounds" not in hdr[hdr.index("Not provided: sharded MPPI"):hdr.index("typedef struct rovmpc_mppi_params")]


def test_setters_reject_a_null_handle_without_a_gpu():
    lib = rovmpc.load_library()
    beta = (ctypes.c_double * 3)(0.5, 0.5, 0.5)
    assert lib.rovmpc_set_noise_correlation(None, beta) == -1
    assert lib.rovmpc_mppi_set_bounds(None, None, None) == -1


def test_structs_unchanged():
    from rovmpc._lib import CEMParams, Config, MPPIParams
    assert ctypes.sizeof(MPPIParams) == 40 and ctypes.sizeof(CEMParams) == 120
    names = " ".join(n for n, _ in Config._fields_)
    for word in ("beta", "noise", "bound", "lo", "hi", "box"):
        assert not re.search(rf"\b{word}", names), word
    body = re.search(r"typedef struct rovmpc_config \{(.*?)\} rovmpc_config;", _header(), re.S).group(1)
    assert "beta" not in body and "noise" not in body


# ---- the Python layer checks before it calls the library -------------------------------------------------------------------
class _NoEngine:
    """Stands where rovmpc.mpc.Engine is: a controller that reaches it has passed its own checks."""
    calls = []

    def __init__(self, cfg=None, model=None, **overrides):
        self.cfg = rovmpc.MPCConfig(**overrides) if cfg is None else cfg
        _NoEngine.calls.append(("create",))

    def __getattr__(self, name):
        def call(*a, **k):
            _NoEngine.calls.append((name,) + tuple(np.asarray(v).tolist() for v in a if isinstance(v, (list, tuple, np.ndarray)) and np.size(v) == 3))
        return call


@pytest.fixture
def no_engine(monkeypatch):
    _NoEngine.calls = []
    monkeypatch.setattr(rovmpc.mpc, "Engine", _NoEngine)
    return _NoEngine.calls


def _controllers():
    return [("MPPI", lambda **kw: rovmpc.MPPI(N=4, K=8, **kw)), ("CEM", lambda **kw: rovmpc.CEM(N=4, K=8, **kw)),
            ("BatchedMPPI", lambda **kw: rovmpc.BatchedMPPI(N=4, K=8, B=2, **kw)),
            ("BatchedCEM", lambda **kw: rovmpc.BatchedCEM(N=4, K=8, B=2, **kw))]


@pytest.mark.parametrize("beta", [(0.5, math.nan, 0.5), (0.5, -0.1, 0.5), (1.0, 0.0, 0.0), (0.0, 0.0, math.inf), (0.5, 0.5)])
def test_beta_rejected_before_the_library(no_engine, beta):
    with pytest.raises(ValueError):
        rovmpc._lib.noise_correlation(beta)
    for name, make in _controllers():
        with pytest.raises(ValueError):
            make(beta=beta)
    assert no_engine == []


@pytest.mark.parametrize("lo,hi", [((0.0, 1.0, 0.0), (1.0, 0.5, 1.0)), ((0.0, math.nan, 0.0), (1.0, 1.0, 1.0)),
                                   ((0.0, 0.0, 0.0), (1.0, 1.0, math.nan)), ((0.0, 0.0, 0.0), None), (None, (1.0, 1.0, 1.0)),
                                   ((0.0, 0.0), (1.0, 1.0))])
def test_mppi_box_rejected_before_the_library(no_engine, lo, hi):
    with pytest.raises(ValueError):
        rovmpc._lib.control_box(lo, hi)
    for name, make in _controllers():
        if "MPPI" in name:
            with pytest.raises(ValueError):
                make(lo=lo, hi=hi)
    assert no_engine == []


def test_accepts_the_limits(no_engine):
    assert rovmpc._lib.noise_correlation(None) is None
    assert rovmpc._lib.noise_correlation((0.0, 0.0, 0.0)) == [0.0, 0.0, 0.0]
    assert rovmpc._lib.noise_correlation((0.999, 0.0, 0.5)) == [0.999, 0.0, 0.5]
    assert rovmpc._lib.control_box(None, None) is None
    assert rovmpc._lib.control_box(*NO_BOX) == ([-math.inf] * 3, [math.inf] * 3)
    assert rovmpc._lib.control_box((1.0, -math.inf, 2.0), (1.0, 0.0, math.inf)) == ([1.0, -math.inf, 2.0], [1.0, 0.0, math.inf])
    for name, make in _controllers():
        del no_engine[:]
        box = dict(lo=NO_BOX[0], hi=NO_BOX[1])
        ctl = make(beta=(0.0, 0.999, 0.0), **box)
        assert ctl.beta == [0.0, 0.999, 0.0]
        # one code path: the settings reach the engine from _PlanController, right after it exists
        assert no_engine[0] == ("create",) and no_engine[1] == ("set_noise_correlation", [0.0, 0.999, 0.0]), name
        if "MPPI" in name:
            assert no_engine[2][0] == "mppi_set_bounds", name
        else:
            assert all(c[0] != "mppi_set_bounds" for c in no_engine), name
        del no_engine[:]
        make()                                          # the defaults call neither setter
        assert not [c for c in no_engine if c[0] in ("set_noise_correlation", "mppi_set_bounds")], name


# ---- the restatement checks itself -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def normals():
    from oracle import rovmpc_oracle as orc
    return orc.philox_normals


def test_ref_white_is_the_existing_law(normals):
    K, N = 37, 5
    nu = np.arange(N * 3, dtype=np.float64).reshape(N, 3) * 0.1
    std = (0.5, 0.0, 2.0)
    for dtype in (np.float64, np.float32):
        U = proposal_sample_ref(normals, 11, 7, K, N, std, nu, (0.0, 0.0, 0.0), dtype=dtype)
        assert np.array_equal(U, mppi_sample_ref(normals, 11, 7, K, N, std, nu, dtype=dtype))
        lo, hi = (-0.2, 0.1, -math.inf), (0.9, 0.1, 1.0)
        sigma = np.abs(nu) + 0.1
        U = proposal_sample_ref(normals, 11, 7, K, N, sigma, nu, (0.0, 0.0, 0.0), lo, hi, dtype=dtype)
        assert np.array_equal(U, cem_sample_ref(normals, 11, 7, K, N, sigma, nu, lo, hi, dtype=dtype))


def test_ref_lag_correlation(normals):
    eps = colored_noise(normals, STAT_SEED, 0, STAT_K, STAT_N, STAT_BETA)
    beta = np.asarray(STAT_BETA)
    r1, r3 = lag_correlation(eps, 1), lag_correlation(eps, 3)
    print("lag 1:", r1, "lag 3:", r3)
    assert np.all(np.abs(r1 - beta) <= STAT_BOUND), r1
    assert np.all(np.abs(r3 - beta ** 3) <= STAT_BOUND), r3
    # stationary: unit variance at the first and at the last node
    v = eps[1:].var(axis=0)
    assert np.all(np.abs(v[0] - 1.0) <= 0.1) and np.all(np.abs(v[-1] - 1.0) <= 0.1), (v[0], v[-1])
    # channel 2 (beta = 0) is the white stream itself
    z = normals(STAT_SEED, 0, STAT_K * STAT_N * 3).reshape(STAT_K, STAT_N, 3)
    assert np.array_equal(eps[:, :, 2], z[:, :, 2]) and np.array_equal(eps[:, 0], z[:, 0])


def test_ref_box(normals):
    K, N = 64, 6
    nu = np.tile((0.3, -2.0, 0.05), (N, 1)) + 0.01 * np.arange(N * 3).reshape(N, 3)
    lo, hi = np.array([0.0, -1.0, 0.1]), np.array([0.5, -1.0, math.inf])         # channel 1: lo = hi, below the nominal
    U = proposal_sample_ref(normals, 5, 2, K, N, 3.0 * np.array([0.5, 1.0, 1.0]), nu, (0.9, 0.5, 0.0), lo, hi)
    assert np.all(U >= lo) and np.all(U <= hi)
    assert np.array_equal(U[0], cem_clamp(nu, lo, hi))
    assert np.all(U[:, :, 1] == -1.0)
    assert np.any(U[1:, :, 0] == 0.0) and np.any(U[1:, :, 0] == 0.5) and np.any((U[1:, :, 0] > 0.0) & (U[1:, :, 0] < 0.5))
