"""CEM on the GPU (rovmpc_cem_*): the select-and-refit kernel against the NumPy restatement of include/rovmpc.h, rank
invariance, the sampling law, C2 against the oracle, iterations with the shift, loaded models, isolation from the other entry
points, determinism and errors."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cem_host import cem_clamp, cem_elites, cem_sample_ref, cem_update_ref, shift_mean  # noqa: E402
from plan_controller_helpers import batch_costs_after_step_batch, colmax, defaults, oracle_J, orc, rv  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def same_nan(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- 1. the update kernel against NumPy ------------------------------------------------------------------------------
def _hard_costs(K, E, slice_, rng):
    """NaN, +-inf, a run of ties straddling the E-th cost and a slice boundary, ties at the minimum."""
    J = 10.0 ** rng.uniform(-3.0, 30.0, K)
    if K >= 8:
        J[rng.choice(K, min(K // 8, 500), replace=False)] = np.nan
        J[rng.choice(K, min(K // 16, 200), replace=False)] = np.inf
        J[rng.choice(K, min(K // 16, 200), replace=False)] = -np.inf
        fin = np.flatnonzero(np.isfinite(J))
        J[fin[:: max(len(fin) // 5, 1)][:3]] = J[fin].min()              # ties at the minimum
        srt = np.sort(J[fin])
        t = srt[max(min(E, len(srt)) - 3, 0)]                            # ties at the threshold
        b = min(slice_, K // 2)
        run = np.arange(max(b - 4, 0), min(b + 4, K))                    # across the first slice boundary (or mid-range)
        J[run] = t
        J[rng.choice(K, 4, replace=False)] = t
    return J


CASES = [(1, 20, "f64"), (100, 20, "f32"), (4096, 20, "f64"), (4096, 20, "f32"), (16384, 20, "f64"), (65536, 20, "f32"),
         (262144, 20, "f64"), (5000, 100, "f32"), (9000, 300, "f64"), (300, 300, "f32")]


@pytest.mark.parametrize("K,N,dtype", CASES)
def test_update_kernel_against_numpy(rv, K, N, dtype):
    import torch
    cfg = rv.MPCConfig(N=N, K=K, dtype=dtype)
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(K + N)
    dev = torch.device("cuda", 0)
    slice_ = -(-K // -(-K // 4096))
    with rv.Engine(cfg) as e:
        stream = torch.cuda.current_stream().cuda_stream
        U = (rng.standard_normal((K, N, 3)) * 3.0 + 1.0).astype(cfg.np_dtype)
        dU = torch.tensor(U, device=dev, dtype=tdt)
        mu_in, sg_in = rng.standard_normal((N, 3)), rng.uniform(0.1, 2.0, (N, 3))
        dmu_in, dsg_in = torch.tensor(mu_in, device=dev), torch.tensor(sg_in, device=dev)
        cm = colmax(U, (N, 3))
        for E in sorted({min(E, K) for E in (1, 7, 64, 1024)}):
            alpha, floor = (0.0, (0.0, 0.0, 0.0)) if E % 2 else (0.3, (0.05, 0.0, 0.5))
            p = rv.CEMParams.make(1, E, alpha, (1.0, 1.0, 1.0), floor)
            cases = [_hard_costs(K, E, slice_, rng)]
            if K >= 8:
                few = np.full(K, np.nan)                                  # more elites requested than finite costs
                few[rng.choice(K, max(E // 2, 1), replace=False)] = rng.uniform(0, 1, max(E // 2, 1))
                cases.append(few)
            for J in cases:
                J = J.astype(cfg.np_dtype)
                dJ = torch.tensor(J, device=dev, dtype=tdt)
                outs = []
                for _ in range(2):
                    dmu = torch.full((N, 3), np.nan, device=dev, dtype=torch.float64)
                    dsg = torch.full((N, 3), np.nan, device=dev, dtype=torch.float64)
                    del_ = torch.full((E,), -7, device=dev, dtype=torch.int64)
                    dst = torch.full((4,), -1.0, device=dev, dtype=torch.float64)
                    e.cem_update_device(dJ.data_ptr(), dU.data_ptr(), p, dmu_in.data_ptr(), dsg_in.data_ptr(), dmu.data_ptr(),
                                        dsg.data_ptr(), del_.data_ptr(), dst.data_ptr(), stream)
                    torch.cuda.synchronize()
                    outs.append((dmu.cpu().numpy(), dsg.cpu().numpy(), del_.cpu().numpy(), dst.cpu().numpy()))
                mu, sg, el, st = outs[0]
                mu_r, sg_r, el_r, st_r = cem_update_ref(J, U, E, alpha, floor, mu_in, sg_in)
                assert np.array_equal(el, el_r), (E, el[:10], el_r[:10])
                assert np.all(np.abs(mu - mu_r) <= 1e-12 * cm), (E, np.abs(mu - mu_r).max())
                assert np.all(np.abs(sg - sg_r) <= 1e-12 * cm), (E, np.abs(sg - sg_r).max())
                assert same_nan(st, st_r), (st, st_r)
                # a second run gives the same bits (fixed summation order, no float atomics)
                for a, b in zip(outs[0], outs[1]):
                    assert np.array_equal(a, b, equal_nan=True)
        # no finite cost at all: mean and spread stay bit for bit
        J = np.full(K, np.nan)
        J[1::3] = np.inf
        J[2::3] = -np.inf
        dJ = torch.tensor(J.astype(cfg.np_dtype), device=dev)
        dmu, dsg = torch.empty_like(dmu_in), torch.empty_like(dsg_in)
        del_ = torch.zeros(1, device=dev, dtype=torch.int64)
        dst = torch.zeros(4, device=dev, dtype=torch.float64)
        p = rv.CEMParams.make(1, 1, 0.5, (1.0, 1.0, 1.0), (9.0, 9.0, 9.0))
        e.cem_update_device(dJ.data_ptr(), dU.data_ptr(), p, dmu_in.data_ptr(), dsg_in.data_ptr(), dmu.data_ptr(), dsg.data_ptr(),
                            del_.data_ptr(), dst.data_ptr(), stream)
        torch.cuda.synchronize()
        assert torch.equal(dmu, dmu_in) and torch.equal(dsg, dsg_in)
        assert del_.item() == -1
        st = dst.cpu().numpy()
        assert math.isnan(st[0]) and math.isnan(st[1]) and st[2] == 0.0 and math.isnan(st[3])


# ---- 2. rank invariance ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4096, 16384])
def test_rank_invariance(rv, K):
    """Only the order of the costs matters: J and 2^40 J (exact in f64) give the same bits.  (The exp(-J/lambda) weights of
    MPPI's update change with the scale; this is what CEM adds.)"""
    import torch
    N = 20
    rng = np.random.default_rng(K)
    dev = torch.device("cuda", 0)
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        stream = torch.cuda.current_stream().cuda_stream
        J = _hard_costs(K, 64, 4096, rng)
        dU = torch.tensor(rng.standard_normal((K, N, 3)), device=dev)
        dmu_in = torch.tensor(rng.standard_normal((N, 3)), device=dev)
        dsg_in = torch.tensor(rng.uniform(0.1, 2.0, (N, 3)), device=dev)
        p = rv.CEMParams.make(1, 64, 0.25, (1.0, 1.0, 1.0), (0.01, 0.01, 0.01))
        outs = []
        for scale in (1.0, 2.0 ** 40):
            dJ = torch.tensor(J * scale, device=dev)
            dmu, dsg = torch.empty_like(dmu_in), torch.empty_like(dsg_in)
            del_ = torch.empty(64, device=dev, dtype=torch.int64)
            e.cem_update_device(dJ.data_ptr(), dU.data_ptr(), p, dmu_in.data_ptr(), dsg_in.data_ptr(), dmu.data_ptr(),
                                dsg.data_ptr(), del_.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            outs.append((dmu.cpu(), dsg.cpu(), del_.cpu()))
        for a, b in zip(*outs):
            assert torch.equal(a, b)


# ---- 3. sampling law ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("boxed", [False, True])
def test_sampling_law(rv, orc, dtype, boxed):
    """Iteration 0 samples with sigma = std; iteration 1 of a two-iteration step with the per-node spread the first refit
    gave, which a one-iteration step at the same counter returns."""
    N, K, seed, E = 12, 512, 77, 16
    mean, std = defaults(rv, N)
    mean = mean + 0.01 * np.arange(N * 3).reshape(N, 3)
    lo, hi = ((mean[0] - 1.5 * std), (mean[0] + 0.5 * std)) if boxed else ((-np.inf,) * 3, (np.inf,) * 3)
    T = np.float64 if dtype == "f64" else np.float32
    state, _ = rv.synthetic_problem(K, N)
    one = rv.CEM(N=N, K=K, dtype=dtype, n_elite=E, n_iter=1, seed=seed, mean=mean, lo=lo, hi=hi, alpha=0.2)
    two = rv.CEM(N=N, K=K, dtype=dtype, n_elite=E, n_iter=2, seed=seed, mean=mean, lo=lo, hi=hi, alpha=0.2)
    one.step(state)
    two.step(state)
    U1, _ = one.engine.cem_last()
    U2, _ = two.engine.cem_last()
    mu1, sg1 = one.mean, one.std                        # mu_1, sigma_1 of counter 0 (unshifted)
    assert not np.all(sg1 == sg1[0])                    # a per-node spread
    for U, counter, mu, sg in ((U1, 0, mean, std), (U2, 1, mu1, sg1)):
        assert np.array_equal(U[0], cem_clamp(mu, lo, hi).astype(T))
        Uo = cem_sample_ref(orc.philox_normals, seed, counter, K, N, sg, mu, lo, hi)
        if dtype == "f64":
            np.testing.assert_allclose(U[1:], Uo[1:], rtol=1e-12, atol=1e-12)
        else:
            np.testing.assert_allclose(U[1:], Uo[1:].astype(np.float32), rtol=2e-7, atol=1e-5)
        assert np.all(U >= np.asarray(lo).astype(T)) and np.all(U <= np.asarray(hi).astype(T))
        if boxed:
            assert np.any(U == np.asarray(lo).astype(T)) and np.any(U == np.asarray(hi).astype(T))
    one.close(); two.close()


# ---- 4. C2 against the oracle ----------------------------------------------------------------------------------------
def test_c2_against_oracle(rv, orc):
    N, K, seed, E = 20, 4096, 20250523, 64
    model = rv.default_model()
    cfg = rv.MPCConfig(N=N, K=K)
    mean, std = defaults(rv, N)
    lo, hi = mean[0] - 2.0 * std, mean[0] + 2.0 * std
    state, _ = rv.synthetic_problem(K, N)
    cem = rv.CEM(cfg, model, n_iter=1, seed=seed, lo=lo, hi=hi)
    assert cem.n_elite == E
    u = cem.step(state)
    U, J = cem.engine.cem_last()
    np.testing.assert_allclose(U, cem_sample_ref(orc.philox_normals, seed, 0, K, N, std, mean, lo, hi), rtol=1e-12, atol=1e-12)
    Jo, trajo = oracle_J(orc, cfg, model, state, U)
    fin = np.isfinite(Jo)
    assert np.array_equal(fin, np.isfinite(J))
    np.testing.assert_allclose(J[fin], Jo[fin], rtol=1e-9)
    k = int(np.argmin(np.where(fin, Jo, np.inf)))
    assert cem.last.index == k
    assert cem.last.cost == pytest.approx(Jo[k], rel=1e-9)
    np.testing.assert_allclose(cem.last.traj, trajo[k], rtol=1e-9, atol=1e-13)
    assert np.array_equal(cem.elites, cem_elites(J, E))
    mu_r, sg_r, el_r, st_r = cem_update_ref(J, U, E, 0.0, (0.0, 0.0, 0.0), mean, std)
    cm = colmax(U, (N, 3))
    assert np.all(np.abs(cem.mean - mu_r) <= 1e-12 * cm) and np.all(np.abs(cem.std - sg_r) <= 1e-12 * cm)
    assert np.array_equal(u, cem_clamp(cem.mean[0], lo, hi))
    st = cem.last_stats
    assert [st["J_best"], st["J_worst_elite"], st["n_finite"], st["J0"]] == list(st_r)
    assert st["J_best"] == cem.last.cost
    cem.close()


# ---- 5. iterations and shift ----------------------------------------------------------------------------------------
def test_iterations_and_shift(rv, orc):
    """n_iter = 3 against a host loop: the restated sampler, the rollout (rollout_costs of a second handle) and
    cem_update_device; the counters, sigma restarting from std at every step, the mean shifted by one node."""
    import torch
    N, K, I, E, seed = 20, 256, 3, 16, 5
    model = rv.default_model()
    cfg = rv.MPCConfig(N=N, K=K)
    mean, std = defaults(rv, N)
    lo, hi = mean[0] - 2.0 * std, mean[0] + 2.0 * std
    alpha, floor = 0.1, 0.02 * std
    base, _ = rv.synthetic_problem(K, N)
    cem = rv.CEM(cfg, model, n_elite=E, n_iter=I, seed=seed, alpha=alpha, std_min=floor, lo=lo, hi=hi)
    ref = rv.Engine(rv.MPCConfig(N=N, K=K), model)
    p = rv.CEMParams.make(1, E, alpha, std, floor, lo, hi)
    dev = torch.device("cuda", 0)
    mu = mean.copy()
    for s in range(4):
        state = base.copy()
        state[12] += 0.01 * s; state[13] -= 0.005 * s; state[3:6] *= 1.0 + 0.05 * s
        u = cem.step(state)
        sg = np.broadcast_to(std, (N, 3)).copy()
        for i in range(I):
            Uh = cem_sample_ref(orc.philox_normals, seed, s * I + i, K, N, sg, mu, lo, hi)
            Jh = ref.rollout_costs(state, Uh)
            dmu, dsg = torch.empty((N, 3), device=dev, dtype=torch.float64), torch.empty((N, 3), device=dev, dtype=torch.float64)
            dJ, dU = torch.tensor(Jh, device=dev), torch.tensor(Uh, device=dev)
            dmu_in, dsg_in = torch.tensor(mu, device=dev), torch.tensor(sg, device=dev)
            del_ = torch.empty(E, device=dev, dtype=torch.int64)
            ref.cem_update_device(dJ.data_ptr(), dU.data_ptr(), p, dmu_in.data_ptr(), dsg_in.data_ptr(), dmu.data_ptr(),
                                  dsg.data_ptr(), del_.data_ptr(), 0, 0)
            torch.cuda.synchronize()
            mu, sg, el = dmu.cpu().numpy(), dsg.cpu().numpy(), del_.cpu().numpy()
        U, J = cem.engine.cem_last()
        np.testing.assert_allclose(U, Uh, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(J, Jh, rtol=1e-9)
        assert np.array_equal(cem.elites, el), s
        scale = np.abs(mu).max()
        np.testing.assert_allclose(cem.mean, mu, rtol=0, atol=1e-9 * scale)
        np.testing.assert_allclose(cem.std, sg, rtol=0, atol=1e-9 * scale)
        assert np.array_equal(u, cem_clamp(cem.mean[0], lo, hi))
        k = int(np.argmin(np.where(np.isfinite(J), J, np.inf)))
        assert cem.last.index == k
        mu = shift_mean(cem.mean)                   # the next step starts from the shifted plan the handle kept
    assert cem.step_count == 4
    cem.close(); ref.close()


# ---- 6. loaded models -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["no_builtin", "force_interpreter", "gen2_f32"])
def test_loaded_models(rv, orc, kind):
    N, K, seed, E = 10, 128, 9, 8
    if kind == "gen2_f32":
        model = rv.generation2_model()
        cfg = rv.MPCConfig(N=N, K=K, dtype="f32", feature_map=rv.FEATURES_GEN2)
    else:
        model = rv.default_model()
        cfg = rv.MPCConfig(N=N, K=K, no_builtin=(kind == "no_builtin"), force_interpreter=(kind == "force_interpreter"))
    mean, std = defaults(rv, N)
    state, _ = rv.synthetic_problem(K, N)
    cem = rv.CEM(cfg, model, n_elite=E, n_iter=1, seed=seed, alpha=0.1)
    assert cem.engine.model_path == {"no_builtin": "jit", "force_interpreter": "interpreter", "gen2_f32": "jit"}[kind]
    cem.step(state)
    U, J = cem.engine.cem_last()
    Jo, _ = oracle_J(orc, cfg, model, state, U)
    fin = np.isfinite(Jo)
    k = cem.last.index
    if cfg.dtype == "f64":
        assert np.array_equal(fin, np.isfinite(J))
        np.testing.assert_allclose(J[fin], Jo[fin], rtol=1e-9)
        assert k == int(np.argmin(np.where(fin, Jo, np.inf)))
    else:                                   # the fp32 rule: same k* or |J32 - J64| / J64 < 1e-4
        k64 = int(np.argmin(np.where(fin, Jo, np.inf)))
        assert k == k64 or abs(float(J[k]) - Jo[k64]) / abs(Jo[k64]) < 1e-4
    # the update on the step's own (T) costs and candidates, in double
    mu_r, sg_r, el_r, _ = cem_update_ref(J, U, E, 0.1, (0.0, 0.0, 0.0), mean, std)
    cm = colmax(U, (N, 3))
    assert np.array_equal(cem.elites, el_r)
    assert np.all(np.abs(cem.mean - mu_r) <= 1e-12 * cm) and np.all(np.abs(cem.std - sg_r) <= 1e-12 * cm)
    assert np.array_equal(cem.last.u, cem.mean[0])
    cem.close()


# ---- 7. no disturbance of the other entry points ------------------------------------------------------------------
@pytest.mark.parametrize("force_interp", [False, True])
def test_cem_does_not_disturb_other_steps(rv, force_interp):
    N, K = 12, 256
    cfg = dict(N=N, K=K, force_interpreter=force_interp)
    mean, std = defaults(rv, N)
    state, Ub = rv.synthetic_problem(K, N)
    cp = rv.CEMParams.make(2, 8, 0.1, std)
    mp = rv.MPPIParams.make(2, 0.5, std)
    a, b = rv.Engine(rv.MPCConfig(**cfg)), rv.Engine(rv.MPCConfig(**cfg))
    a.cem_reset(mean)
    a.mppi_reset(mean); b.mppi_reset(mean)
    for s in range(4):
        a.cem_step(state, 1, s, cp)
        ra = a.mpc_step_sampled(state, 42, s, mean[0], std, True).copy()
        rb = b.mpc_step_sampled(state, 42, s, mean[0], std, True).copy()
        assert np.array_equal(ra, rb), s
        a.cem_step(state, 1, 100 + s, cp)
        for x, y in zip(a.mppi_step(state, 3, s, mp), b.mppi_step(state, 3, s, mp)):
            assert np.array_equal(x, y, equal_nan=True), s
        a.cem_step(state, 1, 200 + s, cp)
        sa_, sb_ = a.step(state, Ub), b.step(state, Ub)
        assert sa_.index == sb_.index and sa_.cost == sb_.cost and np.array_equal(sa_.traj, sb_.traj)
        assert np.array_equal(a.rollout_costs(state, Ub), b.rollout_costs(state, Ub))
    assert np.array_equal(a.sampled_candidates(), b.sampled_candidates())
    for x, y in zip(a.mppi_last(), b.mppi_last()):
        assert np.array_equal(x, y, equal_nan=True)
    costs = batch_costs_after_step_batch(a, state, Ub)
    a.cem_step(state, 1, 300, cp)
    assert a.batch_costs_ptr() == costs           # the controller's rollout wrote its own J, not the batched launch's
    a.close(); b.close()


# ---- 8. determinism and errors --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4096, 20000])
def test_determinism(rv, K):
    N = 20
    state, _ = rv.synthetic_problem(K, N)
    out = []
    for _ in range(2):
        m = rv.CEM(N=N, K=K, n_elite=64, n_iter=2, alpha=0.1, seed=11)
        recs = []
        for s in range(6):
            st = state.copy(); st[12] += 1e-3 * s
            m.step(st)
            recs.append((np.concatenate([[m.last.cost, m.last.index], m.last.u, m.last.traj.ravel()]), m.mean.copy(),
                         m.std.copy(), m.elites.copy(), np.array(list(m.last_stats.values()), dtype=np.float64)))
        out.append(recs)
        m.close()
    for r1, r2 in zip(*out):
        for a, b in zip(r1, r2):
            assert np.array_equal(a, b, equal_nan=True)


def test_errors(rv):
    import ctypes as C
    N, K = 8, 64
    state, _ = rv.synthetic_problem(K, N)
    mean, std = defaults(rv, N)
    good = rv.CEMParams.make(1, 4, 0.0, std)
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        with pytest.raises(rv.RovmpcError) as ei:                         # step before reset
            e.cem_step(state, 0, 0, good)
        assert ei.value.code == -1 and "reset" in str(ei.value)
        with pytest.raises(rv.RovmpcError) as ei:                         # nothing to report yet
            e.cem_last()
        assert ei.value.code == -1
        e.cem_reset(mean)
        for field, value in (("struct_size", 40), ("n_iter", 0), ("n_iter", 65), ("n_elite", 0), ("n_elite", K + 1),
                             ("n_elite", 1025), ("reserved", 1), ("alpha", 1.0), ("alpha", -0.5), ("alpha", float("nan"))):
            p = rv.CEMParams.make(1, 4, 0.0, std)
            setattr(p, field, value)
            with pytest.raises(rv.RovmpcError) as ei:
                e.cem_step(state, 0, 0, p)
            assert ei.value.code == -1, (field, value)
            assert e.lib.rovmpc_cem_update_device(e._h, 1, 1, C.byref(p), 1, 1, 1, 1, None, None, None) == -1
        for arr, bad in (("std", float("nan")), ("std", -1.0), ("std_min", float("inf")), ("lo", float("nan")),
                         ("hi", float("nan")), ("lo", 1e300)):
            p = rv.CEMParams.make(1, 4, 0.0, std, lo=(-1e200,) * 3, hi=(1e200,) * 3)
            getattr(p, arr)[1] = bad
            with pytest.raises(rv.RovmpcError) as ei:
                e.cem_step(state, 0, 0, p)
            assert ei.value.code == -1, (arr, bad)
        assert e.lib.rovmpc_cem_update_device(e._h, None, 1, C.byref(good), 1, 1, 1, 1, None, None, None) == -1
        rec, mu, sg, el, st = e.cem_step(state, 0, 0, good)                 # still usable after the refusals
        assert np.isfinite(rec[0]) and np.array_equal(rec[2:5], mu[0]) and st[0] == rec[0]
        assert e.lib.rovmpc_cem_reset(e._h, None) == -1
        e.comm_init(e.comm_unique_id(), 0, 1)
        with pytest.raises(rv.RovmpcError) as ei:
            e.cem_step(state, 0, 1, good)
        assert ei.value.code == -4
        with pytest.raises(rv.RovmpcError) as ei:
            e.cem_reset(mean)
        assert ei.value.code == -4
        e.comm_destroy()
    assert C.sizeof(rv.CEMParams) == 120
