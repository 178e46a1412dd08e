"""CEM on the host side: the C ABI declares the entry points and the parameter struct, the ctypes mirror follows the header,
parameter checks raise before the library is called, and the NumPy restatement of the law (used by test_cem_gpu.py) passes
its own limit checks.  No compute call into the library happens here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import rovmpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CEM_FUNCS = ("rovmpc_cem_reset", "rovmpc_cem_step", "rovmpc_cem_last", "rovmpc_cem_update_device")
INF3 = (math.inf,) * 3


# ---- the law of include/rovmpc.h (rovmpc_cem_step), restated -------------------------------------------------------------
def cem_clamp(v, lo, hi):
    return np.minimum(np.maximum(v, np.asarray(lo, dtype=np.float64)), np.asarray(hi, dtype=np.float64))


def cem_sample_ref(normals, seed, counter, K, N, sigma, mu, lo=(-math.inf,) * 3, hi=INF3, dtype=np.float64):
    """Step 2: U[0] = (T) clamp(mu), U[k] = (T) clamp(mu + sigma z) for k >= 1; `normals` = oracle.philox_normals, sigma (N, 3)
    or (3,)."""
    z = normals(seed, counter, K * N * 3).reshape(K, N, 3)
    mu = np.asarray(mu, dtype=np.float64)
    U = cem_clamp(mu[None] + np.asarray(sigma, dtype=np.float64) * z, lo, hi).astype(dtype)
    U[0] = cem_clamp(mu, lo, hi).astype(dtype)
    return U


def cem_elites(J, n_elite):
    """The first min(n_elite, |F|) of the finite costs ordered by (J_k, k)."""
    J = np.asarray(J, dtype=np.float64).reshape(-1)
    F = np.flatnonzero(np.isfinite(J))
    return F[np.lexsort((F, J[F]))][:n_elite]


def cem_update_ref(J, U, n_elite, alpha, std_min, mu_in, sigma_in):
    """Step 4: (mu_next (N, 3), sigma_next (N, 3), elites (n_elite,) int64 padded with -1, stats (J rank 0, J rank E'-1, |F|,
    J_0)), in float64 whatever the dtype of J and U."""
    J = np.asarray(J, dtype=np.float64).reshape(-1)
    K = J.shape[0]
    mu_in = np.asarray(mu_in, dtype=np.float64)
    sigma_in = np.broadcast_to(np.asarray(sigma_in, dtype=np.float64), mu_in.shape)
    U = np.asarray(U, dtype=np.float64).reshape((K,) + mu_in.shape)
    el = cem_elites(J, n_elite)
    E = len(el)
    elites = np.full(n_elite, -1, dtype=np.int64)
    elites[:E] = el
    nfin = float(np.isfinite(J).sum())
    if E == 0:
        return mu_in.copy(), sigma_in.copy(), elites, np.array([np.nan, np.nan, nfin, J[0]])
    Ue = U[el]
    m = Ue.sum(axis=0) / E
    v = ((Ue - m) ** 2).sum(axis=0) / E
    mu = alpha * mu_in + (1.0 - alpha) * m
    sigma = np.maximum(np.asarray(std_min, dtype=np.float64), alpha * sigma_in + (1.0 - alpha) * np.sqrt(v))
    return mu, sigma, elites, np.array([J[el[0]], J[el[-1]], nfin, J[0]])


def shift_mean(mu):
    return np.vstack([mu[1:], mu[-1:]])


# ---- header and ctypes mirror ----------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "rovmpc.h")) as f:
        return f.read()


def test_header_declares_cem_entry_points():
    hdr = _header()
    declared = set(re.findall(r"\b(rovmpc_[a-z_0-9]+)\s*\(", hdr))
    for name in CEM_FUNCS:
        assert name in declared, name
        assert name in rovmpc.exported_symbols(), name
    assert re.search(r"typedef struct rovmpc_cem_params \{.*?\} rovmpc_cem_params;", hdr, re.S)


def test_cem_params_fields_in_header_order():
    """The ctypes mirror lists the fields of rovmpc_cem_params in the header's order and types; 120 bytes."""
    from rovmpc._lib import CEMParams
    body = re.search(r"typedef struct rovmpc_cem_params \{(.*?)\} rovmpc_cem_params;", _header(), re.S).group(1)
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
    for name, ctype in CEMParams._fields_:
        if ctype is ctypes.c_int32:
            mirror.append((name, "int32_t", 1))
        elif ctype is ctypes.c_double:
            mirror.append((name, "double", 1))
        else:
            mirror.append((name, "double", ctypes.sizeof(ctype) // 8))
    assert fields == [("struct_size", "int32_t", 1), ("n_iter", "int32_t", 1), ("n_elite", "int32_t", 1),
                      ("reserved", "int32_t", 1), ("alpha", "double", 1), ("std", "double", 3), ("std_min", "double", 3),
                      ("lo", "double", 3), ("hi", "double", 3)]
    assert fields == mirror
    assert ctypes.sizeof(CEMParams) == 120


def test_cem_signatures_bound():
    lib = rovmpc.load_library()
    for name in CEM_FUNCS:
        assert getattr(lib, name).restype is ctypes.c_int
    assert len(lib.rovmpc_cem_reset.argtypes) == 2
    assert len(lib.rovmpc_cem_step.argtypes) == 10
    assert len(lib.rovmpc_cem_last.argtypes) == 3
    assert len(lib.rovmpc_cem_update_device.argtypes) == 11


# ---- parameter checks (before the library is called) ------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
BAD = [dict(n_iter=0), dict(n_iter=65), dict(n_iter=1.5), dict(n_elite=0), dict(n_elite=1025),
       dict(alpha=-1e-3), dict(alpha=1.0), dict(alpha=NAN), dict(alpha=INF),
       dict(std=(1.0, -1e-3, 1.0)), dict(std=(1.0, NAN, 1.0)), dict(std=(1.0, INF, 1.0)), dict(std=(1.0, 1.0)),
       dict(std_min=(0.0, 0.0, -1.0)), dict(std_min=(NAN, 0.0, 0.0)),
       dict(lo=(0.0, 2.0, 0.0), hi=(1.0, 1.0, 1.0)), dict(lo=(NAN, 0.0, 0.0)), dict(hi=(1.0, NAN, 1.0)),
       dict(reserved=1)]


@pytest.mark.parametrize("kw", BAD)
def test_cem_params_rejects(kw):
    args = dict(n_iter=1, n_elite=4, alpha=0.0, std=(0.1, 0.1, 0.1))
    args.update(kw)
    with pytest.raises(ValueError):
        rovmpc.CEMParams.make(**args)
    # the controller checks them before it creates a handle (and so before any GPU is needed)
    with pytest.raises(ValueError):
        rovmpc.CEM(N=4, K=2048, **args)


@pytest.mark.parametrize("n_elite", [9, 2048])
def test_cem_class_rejects_more_elites_than_candidates(n_elite):
    with pytest.raises(ValueError):
        rovmpc.CEM(N=4, K=8, n_elite=n_elite)


def test_cem_params_accepts_limits():
    p = rovmpc.CEMParams.make(n_iter=64, n_elite=1024, alpha=0.0, std=(0.0, 0.0, 0.0))
    assert p.struct_size == ctypes.sizeof(rovmpc.CEMParams) == 120 and p.n_iter == 64 and p.n_elite == 1024
    assert p.reserved == 0 and list(p.lo) == [-INF] * 3 and list(p.hi) == [INF] * 3
    p = rovmpc.CEMParams.make(n_iter=1, n_elite=1, alpha=0.999, std=(1.0, 2.0, 3.0), std_min=(0.5, 0.0, 0.0),
                              lo=(-1.0, 0.0, 2.0), hi=(1.0, 0.0, INF))
    assert list(p.std) == [1.0, 2.0, 3.0] and list(p.std_min) == [0.5, 0.0, 0.0]
    assert list(p.lo) == [-1.0, 0.0, 2.0] and list(p.hi) == [1.0, 0.0, INF] and p.alpha == 0.999


def test_cem_class_exported():
    assert rovmpc.CEM is rovmpc.mpc.CEM
    assert rovmpc.CEMParams is rovmpc._lib.CEMParams


# ---- the restatement checks itself -----------------------------------------------------------------------------------
def _problem(K=64, N=5, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 10.0, K), rng.standard_normal((K, N, 3)), rng.standard_normal((N, 3)), rng.uniform(0.5, 2, (N, 3))


def test_ref_all_finite_rows_alpha_0_is_mean_and_population_std():
    J, U, mu, sg = _problem()
    J[[3, 7, 11]] = [np.nan, np.inf, -np.inf]
    keep = np.isfinite(J)
    mu1, sg1, el, st = cem_update_ref(J, U, int(keep.sum()), 0.0, (0.0, 0.0, 0.0), mu, sg)
    np.testing.assert_allclose(mu1, U[keep].mean(axis=0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(sg1, U[keep].std(axis=0), rtol=0, atol=1e-14)
    assert sorted(el) == list(np.flatnonzero(keep))
    assert st[0] == J[keep].min() and st[1] == J[keep].max() and st[2] == keep.sum() and st[3] == J[0]


def test_ref_one_elite_is_the_argmin_with_the_floor():
    J, U, mu, sg = _problem()
    k = int(np.argmin(J))
    floor = (0.25, 0.0, 3.0)
    mu1, sg1, el, st = cem_update_ref(J, U, 1, 0.0, floor, mu, sg)
    assert np.array_equal(mu1, U[k]) and list(el) == [k]
    assert np.array_equal(sg1, np.broadcast_to(floor, sg1.shape))
    # smoothing mixes the old mean and spread in
    mu2, sg2, _, _ = cem_update_ref(J, U, 1, 0.5, (0.0, 0.0, 0.0), mu, sg)
    np.testing.assert_allclose(mu2, 0.5 * mu + 0.5 * U[k], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sg2, 0.5 * sg, rtol=0, atol=1e-15)


def test_ref_ties_at_the_threshold_take_the_lowest_indices():
    J, U, mu, sg = _problem(K=12)
    J[:] = [5.0, 1.0, 3.0, 3.0, 9.0, 3.0, 0.5, 3.0, 7.0, -0.0, 0.0, 3.0]
    _, _, el, st = cem_update_ref(J, U, 6, 0.0, (0.0, 0.0, 0.0), mu, sg)
    assert list(el) == [9, 10, 6, 1, 2, 3]            # -0 and +0 tie: lower index first
    assert st[0] == 0.0 and st[1] == 3.0
    _, _, el, _ = cem_update_ref(J, U, 8, 0.0, (0.0, 0.0, 0.0), mu, sg)
    assert list(el) == [9, 10, 6, 1, 2, 3, 5, 7]


def test_ref_more_elites_than_finite_costs_pads():
    J, U, mu, sg = _problem(K=8)
    J[[0, 2, 4, 6]] = np.nan
    _, _, el, st = cem_update_ref(J, U, 6, 0.0, (0.0, 0.0, 0.0), mu, sg)
    assert list(el[:4]) == list(cem_elites(J, 6)) and list(el[4:]) == [-1, -1] and st[2] == 4.0
    assert math.isnan(st[3])


def test_ref_no_finite_cost_keeps_mean_and_spread():
    J, U, mu, sg = _problem()
    J[:] = np.nan
    J[1::3] = np.inf
    J[2::3] = -np.inf
    mu1, sg1, el, st = cem_update_ref(J, U, 5, 0.3, (9.0, 9.0, 9.0), mu, sg)
    assert np.array_equal(mu1, mu) and mu1 is not mu and np.array_equal(sg1, sg)
    assert list(el) == [-1] * 5
    assert math.isnan(st[0]) and math.isnan(st[1]) and st[2] == 0.0 and math.isnan(st[3])


def test_ref_rank_invariance():
    J, U, mu, sg = _problem()
    a = cem_update_ref(J, U, 7, 0.2, (0.1, 0.1, 0.1), mu, sg)
    b = cem_update_ref(np.exp(J) * 2.0 ** 40, U, 7, 0.2, (0.1, 0.1, 0.1), mu, sg)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)


def test_ref_samples_in_the_box():
    from oracle import rovmpc_oracle as orc
    K, N = 64, 4
    mu = np.arange(N * 3, dtype=np.float64).reshape(N, 3) - 5.0
    sg = np.full((N, 3), 3.0)
    sg[:, 2] = 0.0
    lo, hi = (-2.0, -math.inf, 0.0), (2.0, 4.0, 1.0)
    U = cem_sample_ref(orc.philox_normals, 11, 7, K, N, sg, mu, lo, hi)
    assert np.all(U >= np.array(lo)) and np.all(U <= np.array(hi))
    assert np.array_equal(U[0], cem_clamp(mu, lo, hi))
    z = orc.philox_normals(11, 7, K * N * 3).reshape(K, N, 3)
    np.testing.assert_allclose(U[1:], cem_clamp(mu + sg * z[1:], lo, hi), rtol=0, atol=1e-12)
    # infinite bounds: the identity
    U2 = cem_sample_ref(orc.philox_normals, 11, 7, K, N, sg, mu)
    np.testing.assert_allclose(U2[1:], mu + sg * z[1:], rtol=0, atol=1e-12)
    assert np.array_equal(U2[0], mu)
    assert np.array_equal(shift_mean(mu), np.vstack([mu[1:], mu[-1:]]))
