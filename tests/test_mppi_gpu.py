"""MPPI on the GPU (rovmpc_mppi_*): the update kernel against the NumPy restatement of include/rovmpc.h, the sampling law,
C2 against the oracle, iterations with the shift, the lambda limits, loaded models, isolation from the other entry points,
determinism and errors."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mppi_host import mppi_sample_ref, mppi_update_ref, shift_nominal  # noqa: E402
from plan_controller_helpers import batch_costs_after_step_batch, colmax, defaults, oracle_J, orc, rv  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def nu_tol(J, U, lam, rel_J=1e-9):
    """Bound on |nu - nu_ref| when the two sides' costs differ by rel_J |J|: a weight moves by about rel_J |J| / lambda
    relative, for every candidate whose weight is not zero."""
    J = np.asarray(J, dtype=np.float64)
    fin = np.isfinite(J)
    live = fin & ((J - J[fin].min()) / lam < 745.0)
    d = rel_J * np.abs(J[live]).max() / lam
    scale = np.abs(np.asarray(U, dtype=np.float64)).max()
    return 4.0 * d * scale + 1e-12 * scale


def lam_for(J):
    """A temperature on the scale of the costs' spread (so the weights neither collapse nor flatten)."""
    J = np.asarray(J, dtype=np.float64)
    J = J[np.isfinite(J)]
    return float(max(np.median(J - J.min()), 1e-12))


# ---- 1. the update kernel against NumPy ------------------------------------------------------------------------------
def _hard_costs(K, rng):
    J = 10.0 ** rng.uniform(-3.0, 30.0, K)
    if K >= 8:
        J[rng.choice(K, min(K // 8, 500), replace=False)] = np.nan
        J[rng.choice(K, min(K // 16, 200), replace=False)] = np.inf
        J[rng.choice(K, min(K // 16, 200), replace=False)] = -np.inf
        fin = np.flatnonzero(np.isfinite(J))
        lo = J[fin].min()
        J[fin[:: max(len(fin) // 5, 1)][:5]] = lo         # ties at the minimum
        J[fin[-3:]] = lo + rng.uniform(0.0, 10.0, 3)
    return J


@pytest.mark.parametrize("K,N", [(1, 20), (100, 20), (4096, 20), (16384, 20), (1000, 100), (300, 300)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_update_kernel_against_numpy(rv, K, N, dtype):
    import torch
    cfg = rv.MPCConfig(N=N, K=K, dtype=dtype)
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(K + N)
    dev = torch.device("cuda", 0)
    with rv.Engine(cfg) as e:
        stream = torch.cuda.current_stream().cuda_stream
        for lam in (1e-6, 0.5, 1e8):
            J = _hard_costs(K, rng).astype(cfg.np_dtype)
            U = (rng.standard_normal((K, N, 3)) * 3.0 + 1.0).astype(cfg.np_dtype)
            nu_in = rng.standard_normal((N, 3))
            dJ, dU = torch.tensor(J, device=dev, dtype=tdt), torch.tensor(U, device=dev, dtype=tdt)
            dnu_in = torch.tensor(nu_in, device=dev)
            dnu_out = torch.full((N, 3), np.nan, device=dev, dtype=torch.float64)
            dst = torch.full((4,), -1.0, device=dev, dtype=torch.float64)
            e.mppi_update_device(dJ.data_ptr(), dU.data_ptr(), lam, dnu_in.data_ptr(), dnu_out.data_ptr(), dst.data_ptr(), stream)
            torch.cuda.synchronize()
            nu, st = dnu_out.cpu().numpy(), dst.cpu().numpy()
            nu_ref, st_ref = mppi_update_ref(J, U, lam, nu_in)
            assert np.all(np.abs(nu - nu_ref) <= 1e-12 * colmax(U, (N, 3))), (lam, np.abs(nu - nu_ref).max())
            assert st[0] == st_ref[0]
            assert st[1] == pytest.approx(st_ref[1], rel=1e-12) and st[2] == pytest.approx(st_ref[2], rel=1e-12)
            assert st[3] == st_ref[3] or (math.isnan(st[3]) and math.isnan(st_ref[3]))
            # a second run gives the same bits (fixed summation order, no float atomics)
            dnu2 = torch.empty_like(dnu_out)
            e.mppi_update_device(dJ.data_ptr(), dU.data_ptr(), lam, dnu_in.data_ptr(), dnu2.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            assert torch.equal(dnu2, dnu_out)
        # no finite cost at all: the nominal stays bit for bit
        J = np.full(K, np.nan)
        J[1::3] = np.inf
        J[2::3] = -np.inf
        dJ = torch.tensor(J.astype(cfg.np_dtype), device=dev)
        e.mppi_update_device(dJ.data_ptr(), dU.data_ptr(), 0.5, dnu_in.data_ptr(), dnu_out.data_ptr(), dst.data_ptr(), stream)
        torch.cuda.synchronize()
        assert torch.equal(dnu_out, dnu_in)
        st = dst.cpu().numpy()
        assert math.isnan(st[0]) and st[1] == 0.0 and st[2] == 0.0 and math.isnan(st[3])


# ---- 2. sampling law ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sampling_law(rv, orc, dtype):
    N, K = 12, 256
    nu, std = defaults(rv, N)
    nu = nu + 0.01 * np.arange(N * 3).reshape(N, 3)
    mppi = rv.MPPI(N=N, K=K, dtype=dtype, lam=1.0, n_iter=1, seed=77, nominal=nu)
    state, _ = rv.synthetic_problem(K, N)
    for s in range(2):
        nu_before = nu if s == 0 else shift_nominal(mppi.nominal)
        mppi.step(state)
        U, _ = mppi.engine.mppi_last()
        T = np.float64 if dtype == "f64" else np.float32
        assert np.array_equal(U[0], nu_before.astype(T))
        Uo = mppi_sample_ref(orc.philox_normals, 77, s, K, N, std, nu_before)
        if dtype == "f64":
            np.testing.assert_allclose(U[1:], Uo[1:], rtol=1e-12, atol=1e-9)
        else:
            np.testing.assert_allclose(U[1:], Uo[1:].astype(np.float32), rtol=2e-7, atol=1e-5)
    mppi.close()


# ---- 3. C2 against the oracle ----------------------------------------------------------------------------------------
def test_c2_against_oracle(rv, orc):
    N, K, seed = 20, 4096, 20250523
    model = rv.default_model()
    cfg = rv.MPCConfig(N=N, K=K)
    nu, std = defaults(rv, N)
    state, _ = rv.synthetic_problem(K, N)
    Uh = mppi_sample_ref(orc.philox_normals, seed, 0, K, N, std, nu)
    Jh, _ = oracle_J(orc, cfg, model, state, Uh)
    lam = lam_for(Jh)
    mppi = rv.MPPI(cfg, model, lam=lam, n_iter=1, seed=seed)
    u = mppi.step(state)
    U, J = mppi.engine.mppi_last()
    np.testing.assert_allclose(U, Uh, rtol=1e-12, atol=1e-9)
    Jo, trajo = oracle_J(orc, cfg, model, state, U)
    fin = np.isfinite(Jo)
    assert np.array_equal(fin, np.isfinite(J))
    np.testing.assert_allclose(J[fin], Jo[fin], rtol=1e-9)
    k = int(np.argmin(np.where(fin, Jo, np.inf)))
    assert mppi.last.index == k
    assert mppi.last.cost == pytest.approx(Jo[k], rel=1e-9)
    np.testing.assert_allclose(mppi.last.traj, trajo[k], rtol=1e-9, atol=1e-13)
    assert np.array_equal(u, mppi.nominal[0])
    nu_ref, st_ref = mppi_update_ref(Jo, U, lam, nu)
    assert np.abs(mppi.nominal - nu_ref).max() <= nu_tol(Jo, U, lam)
    # against its own costs the update is exact to rounding
    nu_own, st_own = mppi_update_ref(J, U, lam, nu)
    assert np.abs(mppi.nominal - nu_own).max() <= 1e-12 * np.abs(U).max()
    st = mppi.last_stats
    assert st["rho"] == J[fin].min() and st["J0"] == J[0]
    assert st["eta"] == pytest.approx(st_own[1], rel=1e-12) and st["ess"] == pytest.approx(st_own[2], rel=1e-12)
    assert 1.0 <= st["ess"] <= K
    mppi.close()


# ---- 4. iterations and shift ----------------------------------------------------------------------------------------
def test_iterations_and_shift(rv, orc):
    N, K, I, seed = 20, 256, 3, 5
    model = rv.default_model()
    cfg = rv.MPCConfig(N=N, K=K)
    nu0, std = defaults(rv, N)
    std = 0.5 * std
    base, _ = rv.synthetic_problem(K, N)
    states = []
    for s in range(5):
        st = base.copy()
        st[12] += 0.01 * s; st[13] -= 0.005 * s; st[3:6] *= 1.0 + 0.05 * s
        states.append(st)
    Jh, _ = oracle_J(orc, cfg, model, states[0], mppi_sample_ref(orc.philox_normals, seed, 0, K, N, std, nu0))
    lam = lam_for(Jh)
    mppi = rv.MPPI(cfg, model, lam=lam, std=std, n_iter=I, seed=seed)
    nu = nu0.copy()
    tol = 0.0
    for s, state in enumerate(states):
        u = mppi.step(state)
        for i in range(I):
            U = mppi_sample_ref(orc.philox_normals, seed, s * I + i, K, N, std, nu)
            Jo, trajo = oracle_J(orc, cfg, model, state, U)
            nu_next, st_ref = mppi_update_ref(Jo, U, lam, nu)
            tol = 2.0 * tol + nu_tol(Jo, U, lam)             # an error of the nominal carries into the next draw
            nu = nu_next
        scale = np.abs(nu).max()
        assert np.abs(mppi.nominal - nu).max() <= tol + 1e-9 * scale, (s, np.abs(mppi.nominal - nu).max(), tol)
        np.testing.assert_allclose(u, nu[0], rtol=0, atol=tol + 1e-9 * scale)
        assert np.array_equal(u, mppi.nominal[0])
        st = mppi.last_stats
        assert st["rho"] == pytest.approx(st_ref[0], rel=1e-7)
        assert st["J0"] == pytest.approx(st_ref[3], rel=1e-7)
        assert st["eta"] == pytest.approx(st_ref[1], rel=1e-5) and st["ess"] == pytest.approx(st_ref[2], rel=1e-5)
        fin = np.isfinite(Jo)
        k = int(np.argmin(np.where(fin, Jo, np.inf)))
        assert mppi.last.index == k
        np.testing.assert_allclose(mppi.last.traj, trajo[k], rtol=1e-7, atol=1e-10)
        nu = shift_nominal(mppi.nominal)            # the next step starts from the shifted plan the handle kept
    assert mppi.step_count == 5
    mppi.close()


# ---- 5. limits ------------------------------------------------------------------------------------------------------
def test_lambda_limits(rv):
    N, K = 12, 512
    state, _ = rv.synthetic_problem(K, N)
    lo = rv.MPPI(N=N, K=K, lam=1e-300, n_iter=1, seed=3)
    lo.step(state)
    U, J = lo.engine.mppi_last()
    fin = np.isfinite(J)
    k = int(np.argmin(np.where(fin, J, np.inf)))
    assert np.sum(J == J[k]) == 1
    assert np.array_equal(lo.nominal, U[k]) and lo.last.index == k
    assert lo.last_stats["eta"] == 1.0 and lo.last_stats["ess"] == 1.0
    lo.close()
    hi = rv.MPPI(N=N, K=K, lam=1e300, n_iter=1, seed=3)
    hi.step(state)
    U, J = hi.engine.mppi_last()
    fin = np.isfinite(J)
    np.testing.assert_allclose(hi.nominal, U[fin].mean(axis=0), rtol=0, atol=1e-12 * np.abs(U).max())
    assert hi.last_stats["eta"] == fin.sum()
    hi.close()


# ---- 6. loaded models -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["no_builtin", "force_interpreter", "gen2_f32"])
def test_loaded_models(rv, orc, kind):
    N, K, seed = 10, 128, 9
    if kind == "gen2_f32":
        model = rv.generation2_model()
        cfg = rv.MPCConfig(N=N, K=K, dtype="f32", feature_map=rv.FEATURES_GEN2)
    else:
        model = rv.default_model()
        cfg = rv.MPCConfig(N=N, K=K, no_builtin=(kind == "no_builtin"), force_interpreter=(kind == "force_interpreter"))
    nu, std = defaults(rv, N)
    state, _ = rv.synthetic_problem(K, N)
    Uh = mppi_sample_ref(orc.philox_normals, seed, 0, K, N, std, nu)
    Jh, _ = oracle_J(orc, cfg, model, state, Uh)
    lam = lam_for(Jh)
    mppi = rv.MPPI(cfg, model, lam=lam, n_iter=1, seed=seed)
    assert mppi.engine.model_path == {"no_builtin": "jit", "force_interpreter": "interpreter", "gen2_f32": "jit"}[kind]
    mppi.step(state)
    U, J = mppi.engine.mppi_last()
    Jo, _ = oracle_J(orc, cfg, model, state, U)
    fin = np.isfinite(Jo)
    k = mppi.last.index
    if cfg.dtype == "f64":
        np.testing.assert_allclose(J[fin], Jo[fin], rtol=1e-9)
        assert k == int(np.argmin(np.where(fin, Jo, np.inf)))
        assert np.abs(mppi.nominal - mppi_update_ref(Jo, U, lam, nu)[0]).max() <= nu_tol(Jo, U, lam)
    else:                                   # the fp32 rule: same k* or |J32 - J64| / J64 < 1e-4
        k64 = int(np.argmin(np.where(fin, Jo, np.inf)))
        assert k == k64 or abs(float(J[k]) - Jo[k64]) / abs(Jo[k64]) < 1e-4
    # the update on the step's own (T) costs and candidates, in double
    nu_own, _ = mppi_update_ref(J, U, lam, nu)
    assert np.abs(mppi.nominal - nu_own).max() <= 1e-12 * np.abs(U.astype(np.float64)).max()
    assert np.array_equal(mppi.last.u, mppi.nominal[0])
    mppi.close()


# ---- 7. no disturbance of the other entry points ------------------------------------------------------------------
@pytest.mark.parametrize("force_interp", [False, True])
def test_mppi_does_not_disturb_other_steps(rv, force_interp):
    N, K = 12, 256
    cfg = dict(N=N, K=K, force_interpreter=force_interp)
    nu, std = defaults(rv, N)
    state, Ub = rv.synthetic_problem(K, N)
    params = rv.MPPIParams.make(2, 0.5, std)
    a, b = rv.Engine(rv.MPCConfig(**cfg)), rv.Engine(rv.MPCConfig(**cfg))
    a.mppi_reset(nu)
    for s in range(4):
        a.mppi_step(state, 1, s, params)
        ra = a.mpc_step_sampled(state, 42, s, nu[0], std, True).copy()
        rb = b.mpc_step_sampled(state, 42, s, nu[0], std, True).copy()
        assert np.array_equal(ra, rb), s
        a.mppi_step(state, 1, 100 + s, params)
        sa_, sb_ = a.step(state, Ub), b.step(state, Ub)
        assert sa_.index == sb_.index and sa_.cost == sb_.cost and np.array_equal(sa_.traj, sb_.traj)
        assert np.array_equal(a.rollout_costs(state, Ub), b.rollout_costs(state, Ub))
    assert np.array_equal(a.sampled_candidates(), b.sampled_candidates())
    costs = batch_costs_after_step_batch(a, state, Ub)
    a.mppi_step(state, 1, 200, params)
    assert a.batch_costs_ptr() == costs           # the controller's rollout wrote its own J, not the batched launch's
    a.close(); b.close()


# ---- 8. determinism -------------------------------------------------------------------------------------------------
def test_determinism(rv):
    N, K = 20, 4096
    state, _ = rv.synthetic_problem(K, N)
    out = []
    for _ in range(2):
        m = rv.MPPI(N=N, K=K, lam=0.1, n_iter=2, seed=11)
        recs = []
        for s in range(10):
            st = state.copy(); st[12] += 1e-3 * s
            m.step(st)
            recs.append((np.concatenate([[m.last.cost, m.last.index], m.last.u, m.last.traj.ravel()]), m.nominal.copy(),
                         np.array(list(m.last_stats.values()))))
        out.append(recs)
        m.close()
    for (r1, n1, s1), (r2, n2, s2) in zip(*out):
        assert np.array_equal(r1, r2) and np.array_equal(n1, n2) and np.array_equal(s1, s2, equal_nan=True)


# ---- 9. errors ------------------------------------------------------------------------------------------------------
def test_errors(rv):
    import ctypes as C
    N, K = 8, 64
    state, _ = rv.synthetic_problem(K, N)
    nu, std = defaults(rv, N)
    good = rv.MPPIParams.make(1, 1.0, std)
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        with pytest.raises(rv.RovmpcError) as ei:                         # step before reset
            e.mppi_step(state, 0, 0, good)
        assert ei.value.code == -1 and "reset" in str(ei.value)
        with pytest.raises(rv.RovmpcError) as ei:                         # nothing to report yet
            e.mppi_last()
        assert ei.value.code == -1
        e.mppi_reset(nu)
        for field, value in (("struct_size", 8), ("n_iter", 0), ("n_iter", 65), ("lambda_", 0.0), ("lambda_", -1.0),
                             ("lambda_", float("nan")), ("lambda_", float("inf"))):
            p = rv.MPPIParams.make(1, 1.0, std)
            setattr(p, field, value)
            with pytest.raises(rv.RovmpcError) as ei:
                e.mppi_step(state, 0, 0, p)
            assert ei.value.code == -1, (field, value)
        for bad in (float("nan"), -1.0, float("inf")):
            p = rv.MPPIParams.make(1, 1.0, std)
            p.std[1] = bad
            with pytest.raises(rv.RovmpcError) as ei:
                e.mppi_step(state, 0, 0, p)
            assert ei.value.code == -1
        for lam in (0.0, -1.0, float("nan")):
            assert e.lib.rovmpc_mppi_update_device(e._h, 1, 1, lam, 1, 1, None, None) == -1
        rec, nu1, st = e.mppi_step(state, 0, 0, good)                     # still usable after the refusals
        assert np.isfinite(rec[0]) and np.array_equal(rec[2:5], nu1[0])
        assert e.lib.rovmpc_mppi_reset(e._h, None) == -1
        e.comm_init(e.comm_unique_id(), 0, 1)
        with pytest.raises(rv.RovmpcError) as ei:
            e.mppi_step(state, 0, 1, good)
        assert ei.value.code == -4
        with pytest.raises(rv.RovmpcError) as ei:
            e.mppi_reset(nu)
        assert ei.value.code == -4
        e.comm_destroy()
    assert C.sizeof(rv.MPPIParams) == 40
