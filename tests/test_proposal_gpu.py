"""The shaped proposal of MPPI and CEM on the GPU (rovmpc_set_noise_correlation, rovmpc_mppi_set_bounds): the candidates
against the NumPy restatement of include/rovmpc.h at the shapes where the sampler's tiling can go wrong, the defaults
untouched bit for bit, the MPPI box (candidates, nominal and control inside it exactly; the update against the clamped NumPy
update), batched against single and device loop against host-stepped loop with shaping on, determinism, no disturbance of the
other entry points, the lag-1 correlation of what the device drew, and the error codes."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_controller_helpers import defaults, orc, rv  # noqa: E402,F401
from plan_loop_helpers import assert_rows_equal, host_loop, host_loop_batch, parts_of, record_of, same  # noqa: E402
from test_cem_host import cem_clamp, cem_update_ref, shift_mean  # noqa: E402
from test_mppi_host import mppi_update_ref, shift_nominal  # noqa: E402
from test_proposal_host import (NO_BOX, STAT_BETA, STAT_BOUND, STAT_K, STAT_N, STAT_SEED, lag_correlation,  # noqa: E402
                                proposal_sample_ref, stat_inputs)

pytestmark = pytest.mark.gpu

BETA = (0.9, 0.5, 0.0)
SHAPES = [(1, 20), (37, 5), (256, 12), (1000, 100), (8, 300)]


def np_T(dtype):
    return np.float64 if dtype == "f64" else np.float32


def assert_law(U, Uo, dtype, what=""):
    """The tolerances of test_mppi_gpu.py::test_sampling_law."""
    if dtype == "f64":
        np.testing.assert_allclose(U, Uo, rtol=1e-12, atol=1e-9, err_msg=str(what))
    else:
        np.testing.assert_allclose(U, Uo.astype(np.float32), rtol=2e-7, atol=1e-5, err_msg=str(what))


def plan_of(rv, N):
    mean, std = defaults(rv, N)
    return mean + 0.01 * np.arange(N * 3).reshape(N, 3) / max(N / 12.0, 1.0), std


def box_of(rv, N, width=0.25):
    """A box around the default plan whose bounds are float32 numbers (so that (float) clamp(v) lies inside it too): channel 0
    [m - w, m + w / 2], channel 1 lo = hi, channel 2 bounded below only."""
    mean, std = defaults(rv, N)
    m, w = mean[0], width * std
    lo = np.array([m[0] - w[0], m[1] + 0.1 * w[1], m[2] - 0.5 * w[2]]).astype(np.float32).astype(np.float64)
    hi = np.array([m[0] + 0.5 * w[0], lo[1], math.inf]).astype(np.float32).astype(np.float64)
    return lo, hi


# ---- 1. sampling law ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mppi_sampling_law(rv, orc, dtype, K, N):
    nu, std = plan_of(rv, N)
    mppi = rv.MPPI(N=N, K=K, dtype=dtype, lam=1.0, n_iter=1, seed=77, nominal=nu, beta=BETA)
    state, _ = rv.synthetic_problem(K, N)
    for s in range(2):
        nu_before = nu if s == 0 else shift_nominal(mppi.nominal)
        mppi.step(state)
        U, _ = mppi.engine.mppi_last()
        assert U.shape == (K, N, 3) and np.array_equal(U[0], nu_before.astype(np_T(dtype)))
        assert_law(U, proposal_sample_ref(orc.philox_normals, 77, s, K, N, std, nu_before, BETA), dtype, (s, K, N))
    mppi.close()


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cem_sampling_law(rv, orc, dtype, K, N):
    """Two steps of two iterations.  Iteration 0 of a step draws with sigma = std around the kept mean; a one-iteration step
    at the same counter from the same mean gives its U and J, and the NumPy refit of those gives the per-node spread and the
    mean that iteration 1 draws with."""
    seed, E, alpha = 77, min(8, K), 0.2
    mean, std = plan_of(rv, N)
    lo, hi = mean[0] - 1.5 * std, mean[0] + 0.5 * std
    std_min = 0.02 * std
    state, _ = rv.synthetic_problem(K, N)
    cfg = rv.MPCConfig(N=N, K=K, dtype=dtype)
    p1 = rv.CEMParams.make(1, E, alpha, std, std_min, lo, hi)
    p2 = rv.CEMParams.make(2, E, alpha, std, std_min, lo, hi)
    with rv.Engine(cfg) as one, rv.Engine(cfg) as two:
        for e in (one, two):
            e.set_noise_correlation(BETA)
        two.cem_reset(mean)
        mu = mean
        for s in range(2):
            one.cem_reset(mu)
            one.cem_step(state, seed, 2 * s, p1)                    # counter 2 s: iteration 0 of step s
            U0, J0 = one.cem_last()
            assert_law(U0, proposal_sample_ref(orc.philox_normals, seed, 2 * s, K, N, std, mu, BETA, lo, hi), dtype, (s, 0))
            mu1, sg1, _, _ = cem_update_ref(J0, U0, E, alpha, std_min, mu, std)
            _, mu2, _, _, _ = two.cem_step(state, seed, s, p2)
            U1, _ = two.cem_last()                                  # counter 2 s + 1
            assert_law(U1, proposal_sample_ref(orc.philox_normals, seed, 2 * s + 1, K, N, sg1, mu1, BETA, lo, hi), dtype, (s, 1))
            T = np_T(dtype)
            assert np.all(U1 >= lo.astype(T)) and np.all(U1 <= hi.astype(T))
            mu = shift_mean(mu2)


# ---- 2. the defaults are untouched ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cem", [False, True])
def test_default_settings_change_nothing(rv, cem):
    N, K = 12, 256
    nu, std = plan_of(rv, N)
    state, _ = rv.synthetic_problem(K, N)
    kw = dict(N=N, K=K, n_iter=2, seed=5)
    make = (lambda: rv.CEM(n_elite=16, alpha=0.2, mean=nu, **kw)) if cem else (lambda: rv.MPPI(lam=0.5, nominal=nu, **kw))
    a, b = make(), make()
    b.engine.set_noise_correlation((0.0, 0.0, 0.0))
    b.engine.mppi_set_bounds(*NO_BOX)
    for s in range(3):
        st = state.copy(); st[12] += 1e-3 * s
        ua, ub = a.step(st), b.step(st)
        (Ua, Ja), (Ub, Jb) = [(c.engine.cem_last() if cem else c.engine.mppi_last()) for c in (a, b)]
        assert np.array_equal(Ua, Ub) and np.array_equal(Ja, Jb, equal_nan=True) and np.array_equal(ua, ub)
        assert same(record_of(a.last), record_of(b.last))
        for name in (("mean", "std", "elites") if cem else ("nominal",)):
            assert np.array_equal(getattr(a, name), getattr(b, name)), (s, name)
        assert np.array_equal(list(a.last_stats.values()), list(b.last_stats.values()), equal_nan=True)
        if s == 1:                                      # NULL arguments are the defaults too
            b.engine.set_noise_correlation(None)
            b.engine.mppi_set_bounds(None, None)
    a.close(); b.close()


# ---- 3. the MPPI box ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("beta", [BETA, None])
def test_mppi_box(rv, orc, dtype, beta):
    N, K, seed, lam = 12, 300, 9, 0.5
    nu, _ = plan_of(rv, N)
    lo, hi = box_of(rv, N)
    width = np.where(np.isfinite(hi - lo) & (hi > lo), hi - lo, (hi - lo)[0])
    std = 3.0 * width                                   # most samples saturate
    T = np_T(dtype)
    state, _ = rv.synthetic_problem(K, N)
    mppi = rv.MPPI(N=N, K=K, dtype=dtype, lam=lam, std=std, n_iter=1, seed=seed, nominal=nu, beta=beta, lo=lo, hi=hi)
    nu_in = nu
    for s in range(2):
        u = mppi.step(state)
        U, J = mppi.engine.mppi_last()
        Uo = proposal_sample_ref(orc.philox_normals, seed, s, K, N, std, nu_in, beta or (0.0,) * 3, lo, hi)
        assert_law(U, Uo, dtype, s)
        assert np.array_equal(U[0], cem_clamp(nu_in, lo, hi).astype(T))
        for x in (U.astype(np.float64), mppi.nominal, u):
            assert np.all(x >= lo) and np.all(x <= hi)
        assert np.all(U[:, :, 1] == T(lo[1])) and np.all(mppi.nominal[:, 1] == lo[1])
        sat = np.mean((U[1:, :, 0] == T(lo[0])) | (U[1:, :, 0] == T(hi[0])))
        assert sat > 0.5, sat
        nu_ref, st_ref = mppi_update_ref(J, U, lam, nu_in)
        assert np.isfinite(J).any()
        assert np.abs(mppi.nominal - cem_clamp(nu_ref, lo, hi)).max() <= 1e-12 * np.abs(U.astype(np.float64)).max()
        assert np.array_equal(u, mppi.nominal[0])
        nu_in = shift_nominal(mppi.nominal)
    # no finite cost: the kept nominal is the clamped one
    outside = nu + 10.0 * std
    mppi.reset(outside)
    u = mppi.step(np.full(16, np.nan))
    _, J = mppi.engine.mppi_last()
    assert not np.isfinite(J).any()
    assert np.array_equal(mppi.nominal, cem_clamp(outside, lo, hi)) and np.array_equal(u, mppi.nominal[0])
    assert math.isnan(mppi.last_stats["rho"]) and mppi.last_stats["eta"] == 0.0
    mppi.step(state)                                    # the handle kept the clamped nominal, shifted
    U, _ = mppi.engine.mppi_last()
    assert np.array_equal(U[0], shift_nominal(cem_clamp(outside, lo, hi)).astype(T))
    mppi.close()


@pytest.mark.parametrize("K,N", [(100, 20), (300, 100)])
def test_mppi_update_device_applies_the_box(rv, K, N):
    """rovmpc_mppi_update_device on buffers of the caller's: one column per thread (3 N <= 256) and four."""
    import torch
    from test_mppi_gpu import _hard_costs
    rng = np.random.default_rng(K + N)
    dev = torch.device("cuda", 0)
    lo, hi = np.array([-1.0, 0.25, -math.inf]), np.array([0.5, 0.25, 2.0])
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        e.mppi_set_bounds(lo, hi)
        stream = torch.cuda.current_stream().cuda_stream
        U = rng.standard_normal((K, N, 3)) * 3.0 + 1.0
        nu_in = rng.standard_normal((N, 3)) * 3.0
        dU, dnu_in = torch.tensor(U, device=dev), torch.tensor(nu_in, device=dev)
        for J, lam in ((_hard_costs(K, rng), 0.5), (_hard_costs(K, rng), 1e8), (np.full(K, np.nan), 0.5)):
            dJ = torch.tensor(J, device=dev)
            dnu = torch.full((N, 3), np.nan, device=dev, dtype=torch.float64)
            e.mppi_update_device(dJ.data_ptr(), dU.data_ptr(), lam, dnu_in.data_ptr(), dnu.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            got, want = dnu.cpu().numpy(), cem_clamp(mppi_update_ref(J, U, lam, nu_in)[0], lo, hi)
            assert np.all(got >= lo) and np.all(got <= hi)
            if np.isfinite(J).any():
                assert np.abs(got - want).max() <= 1e-12 * np.abs(U).max()
            else:
                assert np.array_equal(got, want)


# ---- 4. batched equals single ---------------------------------------------------------------------------------------------
def _shaped_kw(rv, N, cem):
    mean, std = defaults(rv, N)
    lo, hi = box_of(rv, N, 1.0)
    if cem:
        return dict(n_elite=8, n_iter=2, alpha=0.15, std=std, std_min=0.02 * std, lo=lo, hi=hi, beta=BETA)
    return dict(lam=0.05, std=std, n_iter=2, lo=lo, hi=hi, beta=BETA)


def _plan_b(rv, N, b):
    mean, std = defaults(rv, N)
    return mean + 0.05 * std * np.random.default_rng(100 + b).standard_normal((N, 3))


def _state_b(rv, K, N, b, s):
    st, _ = rv.synthetic_problem(K, N)
    st = st.copy()
    st[12] += 0.01 * b + 0.002 * s; st[13] -= 0.005 * b; st[3:6] *= 1.0 + 0.03 * b
    return st


@pytest.mark.parametrize("cem", [False, True])
def test_batched_equals_single(rv, cem):
    B, N, K = 3, 8, 100
    kw = _shaped_kw(rv, N, cem)
    seeds = [11, 2000003, 77]
    plans = np.stack([_plan_b(rv, N, b) for b in range(B)])
    Bat, One, plan_kw = (rv.BatchedCEM, rv.CEM, "mean") if cem else (rv.BatchedMPPI, rv.MPPI, "nominal")
    bat = Bat(N=N, K=K, B=B, seeds=seeds, **{plan_kw: plans}, **kw)
    singles = [One(N=N, K=K, seed=seeds[b], **{plan_kw: plans[b]}, **kw) for b in range(B)]
    names = ("mean", "std", "elites") if cem else ("nominal",)
    for s in range(2):
        st = np.stack([_state_b(rv, K, N, b, s) for b in range(B)])
        u = bat.step(st)
        Ub, Jb = bat.candidates()
        for b, one in enumerate(singles):
            ub = one.step(st[b])
            U1, J1 = one.engine.cem_last() if cem else one.engine.mppi_last()
            assert same(Ub[b], U1) and same(Jb[b], J1), (s, b)
            assert same(bat.records[b], record_of(one.last)) and same(u[b], ub), (s, b)
            for name in names:
                assert same(getattr(bat, name)[b], getattr(one, name)), (s, b, name)
            for k, v in one.last_stats.items():
                assert np.array_equal(np.float64(bat.last_stats[k][b]), np.float64(v), equal_nan=True), (s, b, k)
        assert np.isfinite(Jb).any() and not same(Ub[0], Ub[1])
    bat.close()
    for one in singles:
        one.close()


# ---- 5. device loop equals host-stepped loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("cem", [False, True])
def test_device_loop_equals_host_loop(rv, cem, feedback):
    from rovmpc.closed_loop import closed_loop_inputs
    T, N, K = 4, 8, 128
    kw = _shaped_kw(rv, N, cem)
    make = (lambda: rv.CEM(N=N, K=K, seed=31, mean=_plan_b(rv, N, 0), **kw)) if cem else \
           (lambda: rv.MPPI(N=N, K=K, seed=31, nominal=_plan_b(rv, N, 0), **kw))
    dev, ref = make(), make()
    rows = closed_loop_inputs(dev.engine, 12, T)[0]
    res = dev.run(rows, feedback)
    want, _ = host_loop(ref, rows, feedback, cem)
    assert_rows_equal(res, want, (cem, feedback))
    (Ud, Jd), (Uh, Jh) = [(c.engine.cem_last() if cem else c.engine.mppi_last()) for c in (dev, ref)]
    assert same(Ud, Uh) and same(Jd, Jh)
    if not cem:
        lo, hi = kw["lo"], kw["hi"]
        assert np.all(res.u >= lo) and np.all(res.u <= hi) and np.all(res.plans >= lo) and np.all(res.plans <= hi)
    dev.close(); ref.close()


@pytest.mark.parametrize("cem", [False, True])
def test_batched_device_loop_equals_host_loop(rv, cem):
    from rovmpc.closed_loop import closed_loop_inputs
    T, N, K, B = 4, 8, 128, 2
    kw = _shaped_kw(rv, N, cem)
    plans = np.stack([_plan_b(rv, N, b) for b in range(B)])
    Bat, plan_kw = (rv.BatchedCEM, "mean") if cem else (rv.BatchedMPPI, "nominal")
    make = lambda: Bat(N=N, K=K, B=B, seeds=[5, 6], **{plan_kw: plans}, **kw)        # noqa: E731
    dev, ref = make(), make()
    rows = np.ascontiguousarray(closed_loop_inputs(dev.engine, 12, B * T)[0].reshape(B, T, 16))
    res = dev.run(rows, True)
    assert_rows_equal(res, host_loop_batch(ref, rows, True, cem), cem)
    dev.close(); ref.close()


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cem", [False, True])
def test_determinism(rv, cem):
    N, K = 20, 1000
    kw = _shaped_kw(rv, N, cem)
    state, _ = rv.synthetic_problem(K, N)
    out = []
    for _ in range(2):
        c = rv.CEM(N=N, K=K, seed=11, **kw) if cem else rv.MPPI(N=N, K=K, seed=11, **kw)
        recs = []
        for s in range(3):
            st = state.copy(); st[12] += 1e-3 * s
            c.step(st)
            recs.append((record_of(c.last), (c.mean if cem else c.nominal).copy()) + (c.engine.cem_last() if cem else c.engine.mppi_last()))
        out.append(recs)
        c.close()
    for r1, r2 in zip(*out):
        assert all(same(a, b) for a, b in zip(r1, r2))


# ---- 7. the other entry points are undisturbed --------------------------------------------------------------------------
def test_other_entry_points_undisturbed(rv):
    N, K = 12, 256
    nu, std = defaults(rv, N)
    lo, hi = box_of(rv, N)
    state, Ub = rv.synthetic_problem(K, N)
    mp, cp = rv.MPPIParams.make(2, 0.5, std), rv.CEMParams.make(2, 16, 0.1, std)
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as a, rv.Engine(rv.MPCConfig(N=N, K=K)) as b:
        a.set_noise_correlation(BETA)
        a.mppi_set_bounds(lo, hi)
        a.mppi_reset(nu); a.cem_reset(nu)
        for s in range(3):
            a.mppi_step(state, 1, s, mp)
            ra = a.mpc_step_sampled(state, 42, s, nu[0], std, True).copy()
            rb = b.mpc_step_sampled(state, 42, s, nu[0], std, True).copy()
            assert np.array_equal(ra, rb), s
            a.cem_step(state, 1, s, cp)
            sa_, sb_ = a.step(state, Ub), b.step(state, Ub)
            assert sa_.index == sb_.index and sa_.cost == sb_.cost and np.array_equal(sa_.traj, sb_.traj)
            assert np.array_equal(sa_.u, sb_.u)
        Ua, Ub_ = a.sampled_candidates(), b.sampled_candidates()
        assert np.array_equal(Ua, Ub_)
        assert np.any(Ua[..., 0] > hi[0]) and np.any(Ua[..., 0] < lo[0])        # the shooting step's draw is not boxed


# ---- 8. statistics of what the device drew ------------------------------------------------------------------------------
def test_device_lag_correlation(rv):
    nu, std = stat_inputs(rv)
    mppi = rv.MPPI(N=STAT_N, K=STAT_K, lam=1.0, std=std, n_iter=1, seed=STAT_SEED, nominal=nu, beta=STAT_BETA)
    mppi.step(rv.synthetic_problem(STAT_K, STAT_N)[0])
    U, _ = mppi.engine.mppi_last()
    mppi.close()
    eps = (U - nu[None]) / std
    r1 = lag_correlation(eps, 1)
    print("lag 1 on the device:", r1)
    assert np.all(np.abs(r1 - np.asarray(STAT_BETA)) <= STAT_BOUND), r1


# ---- 9. errors --------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_previous_setting(rv, orc):
    import ctypes as C
    N, K, seed = 8, 64, 3
    nu, std = plan_of(rv, N)
    lo, hi = box_of(rv, N, 1.0)
    state, _ = rv.synthetic_problem(K, N)
    good = rv.MPPIParams.make(1, 1.0, std)
    nan, inf = math.nan, math.inf
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        e.set_noise_correlation(BETA)                   # before the first reset
        e.mppi_set_bounds(lo, hi)
        for beta in ((0.5, nan, 0.5), (0.5, -0.1, 0.5), (1.0, 0.0, 0.0), (0.0, 0.0, inf), (-inf, 0.0, 0.0)):
            with pytest.raises(rv.RovmpcError) as ei:
                e.set_noise_correlation(beta)
            assert ei.value.code == -1 and "beta" in str(ei.value), beta
        for l, h in (((0.0, 1.0, 0.0), (1.0, 0.5, 1.0)), ((0.0, nan, 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (1.0, 1.0, nan)),
                     ((0.0, 0.0, 0.0), None), (None, (1.0, 1.0, 1.0))):
            with pytest.raises(rv.RovmpcError) as ei:
                e.mppi_set_bounds(l, h)
            assert ei.value.code == -1, (l, h)
        assert e.lib.rovmpc_set_noise_correlation(None, None) == -1 and e.lib.rovmpc_mppi_set_bounds(None, None, None) == -1
        # the refused calls changed nothing: the step is the one of (BETA, [lo, hi])
        e.mppi_reset(nu)
        rec, nu1, _ = e.mppi_step(state, seed, 0, good)
        U, _ = e.mppi_last()
        np.testing.assert_allclose(U, proposal_sample_ref(orc.philox_normals, seed, 0, K, N, std, nu, BETA, lo, hi), rtol=1e-12, atol=1e-9)
        assert np.all(nu1 >= lo) and np.all(nu1 <= hi) and np.any(U[1:, :, 0] == lo[0])
        # a new setting between steps holds from the next step; a refusal after it leaves it
        e.set_noise_correlation((0.0, 0.3, 0.0))
        e.mppi_set_bounds(None, None)
        with pytest.raises(rv.RovmpcError):
            e.set_noise_correlation((0.0, 0.3, 1.5))
        with pytest.raises(rv.RovmpcError):
            e.mppi_set_bounds(hi, lo - 1.0)
        e.mppi_step(state, seed, 1, good)
        U, _ = e.mppi_last()
        np.testing.assert_allclose(U, proposal_sample_ref(orc.philox_normals, seed, 1, K, N, std, shift_nominal(nu1), (0.0, 0.3, 0.0)),
                                   rtol=1e-12, atol=1e-9)
    assert C.sizeof(rv.MPPIParams) == 40 and C.sizeof(rv.CEMParams) == 120
