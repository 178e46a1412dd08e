"""MPPI on the host side: the C ABI declares the entry points and the parameter struct, the ctypes mirror follows the
header, parameter checks raise before the library is called, and the NumPy restatement of the update law (used by
test_mppi_gpu.py) passes its own limit checks.  No compute call into the library happens here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import rovmpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPPI_FUNCS = ("rovmpc_mppi_reset", "rovmpc_mppi_step", "rovmpc_mppi_last", "rovmpc_mppi_update_device")


# ---- the law of include/rovmpc.h (rovmpc_mppi_step), restated -----------------------------------------------------------
def mppi_update_ref(J, U, lam, nu_in):
    """Step 4: (nu_next (N, 3), stats (rho, eta, ESS, J_0)), in float64 whatever the dtype of J and U."""
    J = np.asarray(J, dtype=np.float64).reshape(-1)
    K = J.shape[0]
    U = np.asarray(U, dtype=np.float64).reshape(K, -1)
    nu_in = np.asarray(nu_in, dtype=np.float64)
    fin = np.isfinite(J)
    if not fin.any():
        return nu_in.copy(), np.array([np.nan, 0.0, 0.0, J[0]])
    rho = J[fin].min()
    w = np.exp(-(J[fin] - rho) / lam)
    eta = w.sum()
    nu = (w[:, None] * U[fin]).sum(axis=0) / eta
    return nu.reshape(nu_in.shape), np.array([rho, eta, eta * eta / (w * w).sum(), J[0]])


def mppi_sample_ref(normals, seed, counter, K, N, std, nu, dtype=np.float64):
    """Step 2: U[0] = (T) nu, U[k] = (T)(nu + std z) for k >= 1; `normals` = oracle.philox_normals."""
    z = normals(seed, counter, K * N * 3).reshape(K, N, 3)
    nu = np.asarray(nu, dtype=np.float64)
    U = (nu[None] + np.asarray(std, dtype=np.float64) * z).astype(dtype)
    U[0] = nu.astype(dtype)
    return U


def shift_nominal(nu):
    return np.vstack([nu[1:], nu[-1:]])


# ---- header and ctypes mirror ----------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "rovmpc.h")).read()


def test_header_declares_mppi_entry_points():
    hdr = _header()
    declared = set(re.findall(r"\b(rovmpc_[a-z_0-9]+)\s*\(", hdr))
    for name in MPPI_FUNCS:
        assert name in declared, name
        assert name in rovmpc.exported_symbols(), name
    assert re.search(r"typedef struct rovmpc_mppi_params \{.*?\} rovmpc_mppi_params;", hdr, re.S)


def test_mppi_params_fields_in_header_order():
    """The ctypes mirror lists the fields of rovmpc_mppi_params in the header's order and types."""
    from rovmpc._lib import MPPIParams
    body = re.search(r"typedef struct rovmpc_mppi_params \{(.*?)\} rovmpc_mppi_params;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(int32_t|double)\s+(.+)", decl.strip(), re.S)
        if not m:
            continue
        for name in m.group(2).split(","):
            name = name.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", name)
            fields.append((arr.group(1) if arr else name, m.group(1), int(arr.group(2)) if arr else 1))
    mirror = []
    for name, ctype in MPPIParams._fields_:
        name = name.rstrip("_")                  # `lambda` is a Python keyword
        if ctype is ctypes.c_int32:
            mirror.append((name, "int32_t", 1))
        elif ctype is ctypes.c_double:
            mirror.append((name, "double", 1))
        else:
            mirror.append((name, "double", ctypes.sizeof(ctype) // 8))
    assert fields == [("struct_size", "int32_t", 1), ("n_iter", "int32_t", 1), ("lambda", "double", 1), ("std", "double", 3)]
    assert fields == mirror
    assert ctypes.sizeof(MPPIParams) == 40


def test_mppi_signatures_bound():
    lib = rovmpc.load_library()
    for name in MPPI_FUNCS:
        assert getattr(lib, name).restype is ctypes.c_int
    assert len(lib.rovmpc_mppi_step.argtypes) == 8
    assert len(lib.rovmpc_mppi_update_device.argtypes) == 8


def test_config_struct_unchanged():
    """MPPI adds no field to rovmpc_config."""
    from rovmpc._lib import Config
    assert "mppi" not in " ".join(n for n, _ in Config._fields_)


# ---- parameter checks (before the library is called) ------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(lam=0.0), dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")),
                                dict(std=(1.0, float("nan"), 1.0)), dict(std=(1.0, -1e-3, 1.0)), dict(std=(1.0, 1.0)),
                                dict(n_iter=0), dict(n_iter=65), dict(n_iter=1.5)])
def test_mppi_params_rejects(kw):
    args = dict(n_iter=1, lam=1.0, std=(0.1, 0.1, 0.1))
    args.update(kw)
    with pytest.raises(ValueError):
        rovmpc.MPPIParams.make(**args)
    # the controller checks them before it creates a handle (and so before any GPU is needed)
    with pytest.raises(ValueError):
        rovmpc.MPPI(N=4, K=8, **args)


def test_mppi_params_accepts_limits():
    p = rovmpc.MPPIParams.make(n_iter=64, lam=1e-300, std=(0.0, 0.0, 0.0))
    assert p.struct_size == ctypes.sizeof(rovmpc.MPPIParams) and p.n_iter == 64 and p.lambda_ == 1e-300
    p = rovmpc.MPPIParams.make(n_iter=1, lam=1e300, std=(1.0, 2.0, 3.0))
    assert list(p.std) == [1.0, 2.0, 3.0]


def test_mppi_class_exported():
    assert rovmpc.MPPI is rovmpc.mpc.MPPI
    assert rovmpc.MPC is rovmpc.mpc.MPC


# ---- the restatement checks itself -----------------------------------------------------------------------------------
def _problem(K=64, N=5, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 10.0, K), rng.standard_normal((K, N, 3)), rng.standard_normal((N, 3))


def test_ref_small_lambda_is_the_argmin():
    J, U, nu = _problem()
    k = int(np.argmin(J))
    nu1, st = mppi_update_ref(J, U, 1e-300, nu)
    assert np.array_equal(nu1, U[k])
    assert st[0] == J[k] and st[1] == 1.0 and st[2] == 1.0 and st[3] == J[0]


def test_ref_large_lambda_is_the_mean_of_finite_rows():
    J, U, nu = _problem()
    J[[3, 7, 11]] = [np.nan, np.inf, -np.inf]
    keep = np.isfinite(J)
    nu1, st = mppi_update_ref(J, U, 1e300, nu)
    np.testing.assert_allclose(nu1, U[keep].mean(axis=0), rtol=0, atol=1e-14)
    assert st[1] == keep.sum() and st[2] == pytest.approx(keep.sum(), rel=1e-14)


def test_ref_no_finite_cost_keeps_the_nominal():
    J, U, nu = _problem()
    J[:] = np.nan
    J[1::3] = np.inf
    J[2::3] = -np.inf
    nu1, st = mppi_update_ref(J, U, 0.5, nu)
    assert np.array_equal(nu1, nu) and nu1 is not nu
    assert math.isnan(st[0]) and st[1] == 0.0 and st[2] == 0.0 and math.isnan(st[3])


def test_ref_weights_and_ties():
    J, U, nu = _problem(K=4)
    J[:] = [2.0, 1.0, 1.0, 3.0]
    lam = 0.5
    w = np.exp(-(J - 1.0) / lam)
    nu1, st = mppi_update_ref(J, U, lam, nu)
    np.testing.assert_allclose(nu1, np.tensordot(w, U, axes=1) / w.sum(), rtol=1e-15, atol=1e-15)
    assert st[0] == 1.0 and st[1] == pytest.approx(w.sum(), rel=1e-15)
    assert st[2] == pytest.approx(w.sum() ** 2 / (w * w).sum(), rel=1e-15) and st[3] == 2.0


def test_ref_sampling_law():
    from oracle import rovmpc_oracle as orc
    K, N = 16, 4
    nu = np.arange(N * 3, dtype=np.float64).reshape(N, 3)
    std = (0.5, 0.0, 2.0)
    U = mppi_sample_ref(orc.philox_normals, 11, 7, K, N, std, nu)
    z = orc.philox_normals(11, 7, K * N * 3).reshape(K, N, 3)
    assert np.array_equal(U[0], nu)
    np.testing.assert_allclose(U[1:], nu + np.array(std) * z[1:], rtol=0, atol=1e-12)
    assert np.array_equal(U[1:, :, 1], np.broadcast_to(nu[:, 1], (K - 1, N)))
    assert np.array_equal(shift_nominal(nu), np.vstack([nu[1:], nu[-1:]]))
