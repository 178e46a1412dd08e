"""Batched MPPI and CEM on the GPU (rovmpc_*_reset_batch / _step_batch / _last_batch): problem b of a batch against its own
single-problem controller, bit for bit -- records, plans, spreads, elite lists, stats, last candidates and costs -- over
several warm-started control steps; model paths, isolation of a problem without a finite cost, permutation, no disturbance
of (or by) the other entry points, determinism across a re-reset with another B, one anchor against the oracle, errors.

Comparisons are exact.  ``same`` compares the bit patterns, so it also holds where a record carries NaN (np.array_equal on the
values would call two identical NaNs different); the stats are compared with np.array_equal(..., equal_nan=True)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_controller_helpers import defaults, oracle_J, orc, rv  # noqa: E402,F401
from plan_golden_cases import plans_for, problems, seeds_for  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS = 4


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
    return np.array_equal(a.view(bits), b.view(bits))


def same_stats(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def lam_of(rv, cfg_kw, model, std, state, nominal):
    """A temperature on the scale of the costs' spread of one draw, so that the weights neither collapse nor flatten."""
    m = rv.MPPI(rv.MPCConfig(**cfg_kw), model, lam=1.0, std=std, n_iter=1, nominal=nominal)
    m.step(state)
    _, J = m.engine.mppi_last()
    m.close()
    J = np.asarray(J, dtype=np.float64)
    J = J[np.isfinite(J)]
    return float(max(np.median(J - J.min()), 1e-12))


def mppi_stats(c):
    s = c.last_stats
    return np.stack([np.atleast_1d(s[k]).astype(np.float64) for k in ("rho", "eta", "ess", "J0")], axis=-1)


def cem_stats(c):
    s = c.last_stats
    return np.stack([np.atleast_1d(s[k]).astype(np.float64) for k in ("J_best", "J_worst_elite", "n_finite", "J0")], axis=-1)


def record_of(single):
    r = single.last
    return np.concatenate([[r.cost, float(r.index)], r.u, r.traj.ravel()])


def check_mppi(rv, cfg_kw, B, n_iter, model=None, steps=STEPS, states_fn=None, order=None):
    """A batch of B against B single controllers, compared after every control step.  Returns what the batch gave."""
    N, K = cfg_kw["N"], cfg_kw["K"]
    model = model or rv.default_model()
    nominals, std = plans_for(rv, B, N)
    seeds = seeds_for(B)
    states_fn = states_fn or (lambda s: problems(rv, B, K, N, s))
    if order is not None:
        nominals, seeds, inner = nominals[order], [seeds[i] for i in order], states_fn
        states_fn = lambda s: inner(s)[order]                           # noqa: E731
    lam = lam_of(rv, cfg_kw, model, std, problems(rv, 1, K, N, 0)[0], plans_for(rv, 1, N)[0][0])
    bat = rv.BatchedMPPI(rv.MPCConfig(**cfg_kw), model, B=B, lam=lam, std=std, n_iter=n_iter, seeds=seeds, nominal=nominals)
    singles = [rv.MPPI(rv.MPCConfig(**cfg_kw), model, lam=lam, std=std, n_iter=n_iter, seed=seeds[b], nominal=nominals[b])
               for b in range(B)]
    out = []
    for s in range(steps):
        st = states_fn(s)
        u = bat.step(st)
        Ub, Jb = bat.candidates()
        assert u.shape == (B, 3) and bat.records.shape == (B, 5 + 2 * (N + 1)) and len(bat.last) == B
        for b, one in enumerate(singles):
            ub = one.step(st[b])
            U1, J1 = one.engine.mppi_last()
            what = (s, b)
            assert same(bat.records[b], record_of(one)), what
            assert same(u[b], ub), what
            assert same(bat.nominal[b], one.nominal), what
            assert same_stats(mppi_stats(bat)[b], mppi_stats(one)[0]), what
            assert same(Ub[b], U1) and same(Jb[b], J1), what
            assert bat.last[b].index == one.last.index
        out.append((bat.records.copy(), bat.nominal.copy(), mppi_stats(bat), Ub, Jb))
    bat.close()
    for one in singles:
        one.close()
    return out


def check_cem(rv, cfg_kw, B, n_iter, n_elite, model=None, steps=STEPS, states_fn=None, order=None, alpha=0.15):
    N, K = cfg_kw["N"], cfg_kw["K"]
    model = model or rv.default_model()
    means, std = plans_for(rv, B, N)
    seeds = seeds_for(B)
    states_fn = states_fn or (lambda s: problems(rv, B, K, N, s))
    if order is not None:
        means, seeds, inner = means[order], [seeds[i] for i in order], states_fn
        states_fn = lambda s: inner(s)[order]                           # noqa: E731
    mean0 = defaults(rv, N)[0][0]
    kw = dict(n_elite=n_elite, n_iter=n_iter, alpha=alpha, std=std, std_min=0.02 * std, lo=mean0 - 1.2 * std, hi=mean0 + 0.9 * std)
    bat = rv.BatchedCEM(rv.MPCConfig(**cfg_kw), model, B=B, seeds=seeds, mean=means, **kw)
    singles = [rv.CEM(rv.MPCConfig(**cfg_kw), model, seed=seeds[b], mean=means[b], **kw) for b in range(B)]
    T = bat.cfg.np_dtype
    out = []
    for s in range(steps):
        st = states_fn(s)
        u = bat.step(st)
        Ub, Jb = bat.candidates()
        assert u.shape == (B, 3) and bat.elites.shape == (B, n_elite) and bat.elites.dtype == np.int64
        # the box is finite and some candidates sit on it
        assert np.any(Ub == np.asarray(kw["lo"]).astype(T)) and np.any(Ub == np.asarray(kw["hi"]).astype(T))
        for b, one in enumerate(singles):
            ub = one.step(st[b])
            U1, J1 = one.engine.cem_last()
            what = (s, b)
            assert same(bat.records[b], record_of(one)), what
            assert same(u[b], ub), what
            assert same(bat.mean[b], one.mean) and same(bat.std[b], one.std), what
            assert np.array_equal(bat.elites[b], one.elites), what
            assert same_stats(cem_stats(bat)[b], cem_stats(one)[0]), what
            assert same(Ub[b], U1) and same(Jb[b], J1), what
        out.append((bat.records.copy(), bat.mean.copy(), bat.std.copy(), bat.elites.copy(), cem_stats(bat), Ub, Jb))
    bat.close()
    for one in singles:
        one.close()
    return out


# ---- 1. / 2. a batch against B single controllers --------------------------------------------------------------------
@pytest.mark.parametrize("n_iter", [1, 2])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_mppi_batch_equals_singles(rv, B, dtype, n_iter):
    out = check_mppi(rv, dict(N=12, K=512, dtype=dtype), B, n_iter)
    assert np.any(out[-1][2][:, 2] > 1.0)                       # the weights did not collapse to the arg-min


@pytest.mark.parametrize("n_iter", [1, 2])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_cem_batch_equals_singles(rv, B, dtype, n_iter):
    check_cem(rv, dict(N=12, K=512, dtype=dtype), B, n_iter, n_elite=24)


def test_cem_batch_cross_workgroup_select(rv):
    """K = 8192: two workgroups per problem, slab rows and ticket of the problem's own."""
    check_cem(rv, dict(N=20, K=8192), 2, 2, n_elite=96, steps=3)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_wide_rows(rv, dtype):
    """3 N > 256: the four-columns-per-thread instantiation of both updates."""
    cfg = dict(N=90, K=384, dtype=dtype)
    check_mppi(rv, cfg, 2, 2, steps=3)
    check_cem(rv, cfg, 2, 2, n_elite=16, steps=3)


# ---- 3. model paths --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["builtin", "force_interpreter", "gen2_f32", "gen3", "gen3_f32"])
def test_model_paths(rv, kind):
    """(The second-order kinds read the rates (dtheta, dgamma) from slots 14 / 15 of problems(): non-zero in every problem.)"""
    N, K = 10, 128
    if kind == "gen2_f32":
        model, cfg = rv.generation2_model(), dict(N=N, K=K, dtype="f32", feature_map=rv.FEATURES_GEN2)
    elif kind in ("gen3", "gen3_f32"):
        model, cfg = rv.generation3_model(), dict(N=N, K=K, dtype=kind[5:] or "f64", jit=True, feature_map=rv.FEATURES_GEN3)
        assert np.all(problems(rv, 2, K, N, 0)[:, 14:16] != 0.0)
    else:
        model, cfg = rv.default_model(), dict(N=N, K=K, force_interpreter=(kind == "force_interpreter"))
    with rv.Engine(rv.MPCConfig(**cfg), model) as e:
        assert e.model_path == {"builtin": "builtin", "force_interpreter": "interpreter", "gen2_f32": "jit", "gen3": "jit",
                                "gen3_f32": "jit"}[kind]
    check_mppi(rv, cfg, 2, 2, model=model)
    check_cem(rv, cfg, 2, 2, n_elite=8, model=model)


# ---- 4. isolation ----------------------------------------------------------------------------------------------------
def _poisoned(rv, B, K, N, bad):
    def states(s):
        st = problems(rv, B, K, N, s)
        st[bad, 12] = np.nan                                   # theta = NaN: no cost of that problem is finite
        return st
    return states


def test_problem_without_a_finite_cost(rv):
    """It keeps its plan (and spread) bit for bit, reports the stats of the empty case and leaves the others alone: they
    still equal their single-problem runs (check_*), which never saw the poisoned problem."""
    B, K, N, bad = 4, 256, 12, 2
    cfg = dict(N=N, K=K)
    nominals, std = plans_for(rv, B, N)
    out = check_mppi(rv, cfg, B, 2, states_fn=_poisoned(rv, B, K, N, bad), steps=3)
    kept = nominals[bad]
    for rec, nu, stats, U, J in out:
        assert not np.isfinite(J[bad]).any() and np.isfinite(J[np.arange(B) != bad]).any()
        assert same(nu[bad], kept)
        assert np.isnan(stats[bad, 0]) and stats[bad, 1] == 0.0 and stats[bad, 2] == 0.0 and not np.isfinite(stats[bad, 3])
        kept = np.vstack([kept[1:], kept[-1:]])                # the shift still happens
    out = check_cem(rv, cfg, B, 2, n_elite=16, states_fn=_poisoned(rv, B, K, N, bad), steps=3)
    kept = nominals[bad]
    for rec, mu, sg, el, stats, U, J in out:
        assert not np.isfinite(J[bad]).any()
        assert same(mu[bad], kept) and same(sg[bad], np.broadcast_to(std, (N, 3)))
        assert np.all(el[bad] == -1) and np.all(el[np.arange(B) != bad][:, 0] >= 0)
        assert np.isnan(stats[bad, 0]) and np.isnan(stats[bad, 1]) and stats[bad, 2] == 0.0 and not np.isfinite(stats[bad, 3])
        kept = np.vstack([kept[1:], kept[-1:]])


def test_permutation(rv):
    """Permuting the problems of a batch permutes the outputs and changes nothing else."""
    B, cfg = 5, dict(N=12, K=256)
    order = np.array([3, 0, 4, 2, 1])
    a, b = check_mppi(rv, cfg, B, 2, steps=3), check_mppi(rv, cfg, B, 2, steps=3, order=order)
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert same(p[order], q)
    a, b = check_cem(rv, cfg, B, 2, n_elite=16, steps=3), check_cem(rv, cfg, B, 2, n_elite=16, steps=3, order=order)
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert same(p[order], q)


# ---- 5. no disturbance, both directions ----------------------------------------------------------------------------
@pytest.mark.parametrize("force_interp", [False, True])
def test_batched_steps_and_the_other_entry_points(rv, force_interp):
    """Handle `a` interleaves batched controller steps with step, mpc_step_sampled, mppi_step, cem_step and
    step_batch_device; `b` never sees a batched controller step and `c` sees nothing else."""
    import torch
    N, K, B = 12, 256, 3
    cfg = dict(N=N, K=K, force_interpreter=force_interp)
    mean, std = defaults(rv, N)
    plans, _ = plans_for(rv, B, N)
    seeds = np.array(seeds_for(B), dtype=np.uint64)
    state, Ub = rv.synthetic_problem(K, N)
    mp, cp = rv.MPPIParams.make(2, 0.5, std), rv.CEMParams.make(2, 8, 0.1, std)
    a, b, c = (rv.Engine(rv.MPCConfig(**cfg)) for _ in range(3))
    for e in (a, b):
        e.mppi_reset(mean); e.cem_reset(mean)
    for e in (a, c):
        e.mppi_reset_batch(plans); e.cem_reset_batch(plans)
    dev = torch.device("cuda", 0)
    R = a.result_len
    d_states = torch.tensor(problems(rv, B, K, N, 9), device=dev)
    d_U = torch.tensor(np.stack([Ub * (1.0 + 0.01 * i) for i in range(B)]), device=dev)

    def device_batch(e):
        d_res = torch.zeros((B, R), device=dev, dtype=torch.float64)
        e.step_batch_device(B, d_states.data_ptr(), d_U.data_ptr(), d_res.data_ptr(), 0)
        torch.cuda.synchronize()
        return d_res.cpu().numpy()

    for s in range(3):
        st = problems(rv, B, K, N, s)
        for x, y in zip(a.mppi_step_batch(st, seeds, s, mp), c.mppi_step_batch(st, seeds, s, mp)):
            assert same(x, y), s
        ra, rb = a.mpc_step_sampled(state, 42, s, mean[0], std, True).copy(), b.mpc_step_sampled(state, 42, s, mean[0], std, True).copy()
        assert same(ra, rb), s
        for x, y in zip(a.cem_step_batch(st, seeds, s, cp), c.cem_step_batch(st, seeds, s, cp)):
            assert same(x, y), s
        for x, y in zip(a.mppi_step(state, 3, s, mp), b.mppi_step(state, 3, s, mp)):
            assert same(x, y), s
        for x, y in zip(a.cem_step(state, 5, s, cp), b.cem_step(state, 5, s, cp)):
            assert same(x, y), s
        for x, y in zip(a.mppi_last_batch() + a.cem_last_batch(), c.mppi_last_batch() + c.cem_last_batch()):
            assert same(x, y), s
        assert same(device_batch(a), device_batch(b)), s
        sa_, sb_ = a.step(state, Ub), b.step(state, Ub)
        assert sa_.index == sb_.index and sa_.cost == sb_.cost and same(sa_.traj, sb_.traj)
        assert same(a.rollout_costs(state, Ub), b.rollout_costs(state, Ub))
    for x, y in zip(a.mppi_last() + a.cem_last(), b.mppi_last() + b.cem_last()):
        assert same(x, y)
    assert same(a.sampled_candidates(), b.sampled_candidates())
    for e in (a, b, c):
        e.close()


# ---- 6. determinism ---------------------------------------------------------------------------------------------------
def test_determinism_and_re_reset(rv):
    N, K, B = 12, 512, 4
    plans, std = plans_for(rv, B, N)
    seeds = np.array(seeds_for(B), dtype=np.uint64)
    mp, cp = rv.MPPIParams.make(2, 0.3, std), rv.CEMParams.make(2, 16, 0.1, std)

    def run(e):
        e.mppi_reset_batch(plans); e.cem_reset_batch(plans)
        got = []
        for s in range(STEPS):
            st = problems(rv, B, K, N, s)
            got += list(e.mppi_step_batch(st, seeds, s, mp)) + list(e.cem_step_batch(st, seeds, s, cp))
            got += list(e.mppi_last_batch()) + list(e.cem_last_batch())
        return got

    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        first = run(e)
        # another B in between: the buffers are made again, twice
        other, _ = plans_for(rv, 7, N)
        e.mppi_reset_batch(other); e.cem_reset_batch(other)
        e.mppi_step_batch(problems(rv, 7, K, N, 0), np.arange(7, dtype=np.uint64), 0, mp)
        e.cem_step_batch(problems(rv, 7, K, N, 0), np.arange(7, dtype=np.uint64), 0, cp)
        second = run(e)
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        third = run(e)
    for x, y, z in zip(first, second, third):
        assert same(x, y) and same(x, z)


# ---- 7. one anchor outside the library --------------------------------------------------------------------------------
def test_c2_costs_against_the_oracle(rv, orc):
    """Problem B - 1 of a C2-sized batch (N = 20, K = 4096, fp64): its costs against the NumPy oracle on its candidates."""
    N, K, B = 20, 4096, 3
    model = rv.default_model()
    cfg = rv.MPCConfig(N=N, K=K)
    state, _ = rv.synthetic_problem(K, N)
    bat = rv.BatchedMPPI(cfg, model, B=B, lam=1.0, n_iter=1)
    bat.step(np.tile(state, (B, 1)))
    U, J = bat.candidates()
    bat.close()
    Jo, _ = oracle_J(orc, cfg, model, state, U[B - 1])
    fin = np.isfinite(Jo)
    assert fin.all()                        # on the synthetic state the oracle leaves every cost finite (checked on the CPU too)
    assert np.array_equal(fin, np.isfinite(J[B - 1]))
    np.testing.assert_allclose(J[B - 1][fin], Jo[fin], rtol=1e-9)


# ---- 8. errors --------------------------------------------------------------------------------------------------------
def test_errors(rv):
    N, K, B = 8, 64, 2
    plans, std = plans_for(rv, B, N)
    st = problems(rv, B, K, N, 0)
    seeds = np.array(seeds_for(B), dtype=np.uint64)
    mp, cp = rv.MPPIParams.make(1, 1.0, std), rv.CEMParams.make(1, 4, 0.0, std)
    R = 5 + 2 * (N + 1)
    rec = np.full((1025, R), -7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                          # noqa: E731
    big_st, big_seeds = np.tile(st[:1], (1025, 1)), np.arange(1025, dtype=np.uint64)
    big_plans = np.tile(plans[:1], (1025, 1, 1))
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        lib, h = e.lib, e._h

        def refused(rc, code=-1):
            assert rc == code, rc
            assert lib.rovmpc_last_error(h), "no message"
            assert np.all(rec == -7.0)                                  # nothing was written: nothing was launched

        def mstep(B_, st_=st, seeds_=seeds, par=mp, out=rec):
            return lib.rovmpc_mppi_step_batch(h, B_, p(st_), None if seeds_ is None else p(seeds_), 0, C.byref(par),
                                              None if out is None else p(out), None, None)

        def cstep(B_, st_=st, seeds_=seeds, par=cp, out=rec):
            return lib.rovmpc_cem_step_batch(h, B_, p(st_), None if seeds_ is None else p(seeds_), 0, C.byref(par),
                                             None if out is None else p(out), None, None, None, None)

        for step in (mstep, cstep):
            refused(step(B))                                            # a step before the reset
            assert b"reset" in lib.rovmpc_last_error(h)
        for last in (lib.rovmpc_mppi_last_batch, lib.rovmpc_cem_last_batch):
            refused(last(h, None, None))
        for reset in (lib.rovmpc_mppi_reset_batch, lib.rovmpc_cem_reset_batch):
            refused(reset(h, 0, p(plans)))
            refused(reset(h, 1025, p(big_plans)))
            refused(reset(h, B, None))
            assert reset(h, B, p(plans)) == 0
        for step in (mstep, cstep):
            refused(step(B + 1, big_st, big_seeds))                     # B differs from the reset's
            refused(step(0))
            refused(step(1025, big_st, big_seeds))
            refused(step(B, seeds_=None))                               # null seeds
            refused(step(B, out=None))
        bad = rv.MPPIParams.make(1, 1.0, std); bad.struct_size = 8
        refused(mstep(B, par=bad))
        bad = rv.MPPIParams.make(1, 1.0, std); bad.lambda_ = 0.0
        refused(mstep(B, par=bad))
        bad = rv.CEMParams.make(1, 4, 0.0, std); bad.struct_size = 40
        refused(cstep(B, par=bad))
        for n_elite in (0, K + 1, 1025):                                # a bad n_elite
            bad = rv.CEMParams.make(1, 4, 0.0, std); bad.n_elite = n_elite
            refused(cstep(B, par=bad))
        # still usable after the refusals, and the Python layer reports the library's message
        r, nu, stats = e.mppi_step_batch(st, seeds, 0, mp)
        assert np.isfinite(r[:, 0]).all() and same(r[:, 2:5], nu[:, 0])
        r, mu, sg, el, stats = e.cem_step_batch(st, seeds, 0, cp)
        assert np.isfinite(r[:, 0]).all() and same(r[:, 2:5], mu[:, 0]) and np.all(el >= 0)
        with pytest.raises(rv.RovmpcError) as ei:
            e.mppi_step_batch(big_st[:3], big_seeds[:3], 1, mp)
        assert ei.value.code == -1 and "reset" in str(ei.value)
        e.comm_init(e.comm_unique_id(), 0, 1)
        refused(mstep(B), -4)
        refused(cstep(B), -4)
        refused(lib.rovmpc_mppi_reset_batch(h, B, p(plans)), -4)
        refused(lib.rovmpc_cem_reset_batch(h, B, p(plans)), -4)
        e.comm_destroy()
