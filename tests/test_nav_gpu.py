"""The navigation cost of MPPI and CEM on the GPU (rovmpc_set_nav_cost, rovmpc_nav_cost_device; law in include/rovmpc.h):
the term against the 50-digit reference of tests/nav_reference.py within 4x its own running error bound, the MPPI and CEM
steps reading J' = J + C, the batch and device-loop equivalences bit for bit with the cost on, the default path untouched,
the errors, and a closed loop that steers the vehicle to a waypoint."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nav_reference as nr  # noqa: E402
from plan_controller_helpers import colmax, defaults, rv  # noqa: E402,F401
from plan_loop_helpers import assert_rows_equal, host_loop, host_loop_batch, parts_of, record_of, same  # noqa: E402
from test_cem_host import cem_elites, cem_update_ref  # noqa: E402
from test_mppi_host import mppi_update_ref  # noqa: E402

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
WEIGHTS = dict(w_pos=(1e3, 2e3, 5e2), w_term=(1e4, 0.0, 3e3), w_du=(1e-4, 2e-4, 0.0), w_sphere=1e4)
ZERO = dict(w_pos=0.0, w_term=0.0, w_du=0.0, w_sphere=0.0)


def c_of(cfg):
    return cfg.v_scale * cfg.dt


def problem(rv, N, K, dtype, seed=0):
    """A state, candidates of the handle's dtype around the scaler statistics, a track near the mean path with `Tr` rows on
    request, and 8 spheres the paths run through."""
    rng = np.random.default_rng(1000 * N + K + seed)
    m = rv.default_model()
    state, _ = rv.synthetic_problem(1, N)
    U = (m.mean[3:6] + m.scale[3:6] * rng.standard_normal((K, N, 3))).astype(NP[dtype])
    c = 1e-3 / 60.0
    travel = c * 100.0 * N

    def track(Tr):
        return state[3:6] + c * m.mean[3:6] * np.arange(1, Tr + 1)[:, None] + 0.1 * travel * rng.standard_normal((Tr, 3))
    spheres = np.concatenate([state[3:6] + travel * rng.uniform(-1.0, 1.0, (8, 3)), travel * rng.uniform(0.3, 1.0, (8, 1))], axis=1)
    return state, U, track, spheres


@functools.lru_cache(maxsize=None)
def term_reference(N, K, dtype):
    """The variants of one shape and their references, computed once: (state, U, [(name, nav kwargs, track, step, Cs, bound)])."""
    import rovmpc
    state, U, track, spheres = problem(rovmpc, N, K, dtype)
    short = max(N // 2, 1)
    variants = [("no spheres, one row", dict(WEIGHTS, spheres=()), track(1), 0, 0),
                ("one sphere, Tr < N, before the origin", dict(WEIGHTS, spheres=spheres[:1]), track(short), 2, 5),
                ("8 spheres, Tr > N, beyond the end", dict(WEIGHTS, spheres=spheres), track(N + 5), 7 + N + 5 + 3, 7),
                ("Tr > N, step - origin wraps to +3", dict(WEIGHTS, spheres=spheres[:1]), track(N + 5), 1, 2 ** 64 - 2),
                ("all weights zero", dict(ZERO, spheres=spheres[:1]), track(3), 1, 0)]
    out = []
    for name, kw, tr, step, origin in variants:
        Cs, b = nr.nav_cost_ref(state[3:6], U, step, 1e-3 / 60.0, tr, origin=origin, **kw)
        out.append((name, dict(kw, origin=origin), tr, step, Cs, b))
    return state, U, out


# ---- 1. the term against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(1, 1), (2, 5), (11, 67), (20, 130), (340, 9)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_term_against_reference(rv, N, K, dtype):
    state, U, variants = term_reference(N, K, dtype)
    rng = np.random.default_rng(N + K)
    worst = 0.0
    with rv.Engine(rv.MPCConfig(N=N, K=K, dtype=dtype)) as e:
        assert c_of(e.cfg) == 1e-3 / 60.0
        for name, kw, tr, step, Cs, b in variants:
            nav, tracks = rv._lib.nav_cost(tr, **kw)
            e.set_nav_cost(nav, tracks)
            Cg = e.nav_cost(state, U, step)
            ratio, ok = nr.check_C(Cg, Cs, b)
            print(f"N {N} K {K} {dtype} {name}: max |C - C_ref| / bound = {ratio:.3g}")
            assert ok, (name, ratio)
            worst = max(worst, ratio)
            if name == "all weights zero":
                assert np.all(Cg == 0.0)
            else:
                assert np.all(Cg > 0.0)
            # the in-place form, with an inf and a NaN planted
            J = rng.uniform(0.05, 5.0, K).astype(NP[dtype])
            if K >= 5:
                J[1], J[K - 2] = np.inf, np.nan
            C2, Jp = e.nav_cost(state, U, step, J=J)
            assert same(C2, Cg), name
            excess = nr.check_J(Jp, J, Cs, b, NP[dtype])
            assert excess <= 1.0, (name, excess)
            if name == "all weights zero":
                fin = np.isfinite(J)
                assert np.array_equal(Jp[fin], J[fin])
    print(f"N {N} K {K} {dtype}: largest ratio {worst:.3g}")


# ---- 2. MPPI and CEM steps read J' ---------------------------------------------------------------------------------------
def step_problem(rv, dtype):
    N, K = 8, 256
    state, _, track, spheres = problem(rv, N, K, dtype, seed=5)
    nav_kw = dict(WEIGHTS, spheres=spheres[:2], origin=1)
    return N, K, state, track(12), nav_kw


def check_step_costs(rv, ctl, last, state, track, nav_kw, step, dtype):
    """last() against (T)(rollout costs of a plain engine on the reported U + C_ref); returns (U, J', J, Cs, bound)."""
    U, Jp = last()
    with rv.Engine(rv.MPCConfig(N=ctl.cfg.N, K=ctl.cfg.K, dtype=dtype)) as plain:
        J = plain.rollout_costs(state, U)
    Cs, b = nr.nav_cost_ref(state[3:6], U, step, c_of(ctl.cfg), track, **nav_kw)
    assert np.array_equal(np.isfinite(J), np.isfinite(Jp))
    excess = nr.check_J(Jp, J, Cs, b, NP[dtype])
    print("largest |J' - (J + C_ref)| over its allowance:", excess)
    assert excess <= 1.0
    fin = np.isfinite(J)
    assert fin.sum() >= ctl.cfg.K // 2 and np.all(nr.as_float(Cs)[fin] > 0)
    return U, Jp, J, Cs, b


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mppi_step_reads_the_nav_cost(rv, dtype):
    N, K, state, track, nav_kw = step_problem(rv, dtype)
    lam, step = 1.0, 3
    ctl = rv.MPPI(N=N, K=K, dtype=dtype, lam=lam, n_iter=2, seed=9, nav=rv.NavCost(track, **nav_kw))
    ctl.step_count = step
    u = ctl.step(state)
    U, Jp, J, Cs, b = check_step_costs(rv, ctl, ctl.engine.mppi_last, state, track, nav_kw, step, dtype)
    nu_ref, st_ref = mppi_update_ref(Jp, U, lam, np.zeros((N, 3)))
    assert np.abs(ctl.nominal - nu_ref).max() <= 1e-12 * np.abs(U).max()
    assert np.array_equal(u, ctl.nominal[0])
    st = ctl.last_stats
    assert st["rho"] == Jp[np.isfinite(Jp)].min() and st["J0"] == Jp[0]
    assert st["eta"] == pytest.approx(st_ref[1], rel=1e-12) and st["ess"] == pytest.approx(st_ref[2], rel=1e-12)
    assert float(Cs[0]) > 0 and abs(st["J0"] - (float(J[0]) + float(Cs[0]))) <= 4 * b[0] + nr.ulp(st["J0"], NP[dtype])
    ctl.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cem_step_reads_the_nav_cost(rv, dtype):
    N, K, state, track, nav_kw = step_problem(rv, dtype)
    E, step = 16, 3
    _, std = defaults(rv, N)
    ctl = rv.CEM(N=N, K=K, dtype=dtype, n_elite=E, n_iter=2, alpha=0.0, seed=9, nav=rv.NavCost(track, **nav_kw))
    ctl.step_count = step
    ctl.step(state)
    U, Jp, J, Cs, b = check_step_costs(rv, ctl, ctl.engine.cem_last, state, track, nav_kw, step, dtype)
    assert np.array_equal(ctl.elites, cem_elites(Jp, E))
    mu_r, sg_r, el_r, st_r = cem_update_ref(Jp, U, E, 0.0, (0.0, 0.0, 0.0), np.zeros((N, 3)), np.tile(std, (N, 1)))
    cm = colmax(U, (N, 3))
    assert np.all(np.abs(ctl.mean - mu_r) <= 1e-12 * cm) and np.all(np.abs(ctl.std - sg_r) <= 1e-12 * cm)
    st = ctl.last_stats
    assert [st["J_best"], st["J_worst_elite"], st["n_finite"], st["J0"]] == list(st_r)
    assert float(Cs[0]) > 0 and abs(st["J0"] - (float(J[0]) + float(Cs[0]))) <= 4 * b[0] + nr.ulp(st["J0"], NP[dtype])
    ctl.close()


# ---- 3. the equivalences, bit for bit ------------------------------------------------------------------------------------
EQ = dict(N=6, K=256)
B3 = 3


def eq_rows(rv, ctl, T, B=None):
    from rovmpc.closed_loop import closed_loop_inputs
    if B is None:
        return closed_loop_inputs(ctl.engine, 12, T)[0]
    return np.ascontiguousarray(closed_loop_inputs(ctl.engine, 12, B * T)[0].reshape(B, T, 16))


def eq_tracks(rows, Tr):
    """(B, min(Tr, T), 3) from rows (B, T, 16): per problem a track a few millimetres off its measured positions."""
    rng = np.random.default_rng(77)
    return np.stack([r[:Tr, 3:6] + 0.003 * rng.standard_normal((len(r[:Tr]), 3)) for r in rows])


def eq_nav(rv, tracks, origin=0, near=None):
    """The weights and two spheres (beside the first rows of `near`, default the tracks' own) shared by a batch."""
    near = tracks if near is None else near
    sph = np.concatenate([near.reshape(-1, 3)[:2] + 0.002, [[0.004], [0.006]]], axis=1)
    return rv.NavCost(tracks, w_pos=(2e3, 1e3, 3e3), w_term=5e3, w_du=(1e-4, 0.0, 2e-4), w_sphere=1e4, spheres=sph, origin=origin)


def seed_of(b):
    return 1000003 * (b + 1) + 17


def eq_plan(rv, b):
    mean, std = defaults(rv, EQ["N"])
    return mean + 0.05 * std * np.random.default_rng(500 + b).standard_normal((EQ["N"], 3))


def make(rv, cem, nav, b=None, dtype="f64", n_iter=2):
    """A single controller of problem b, or (b None) the batched one of B3 problems."""
    kw = dict(dtype=dtype, n_iter=n_iter, nav=nav, **EQ)
    if cem:
        _, std = defaults(rv, EQ["N"])
        kw.update(n_elite=16, alpha=0.15, std_min=0.02 * std)
    else:
        kw.update(lam=0.5)
    plan = "mean" if cem else "nominal"
    if b is None:
        kw[plan] = np.stack([eq_plan(rv, i) for i in range(B3)])
        return (rv.BatchedCEM if cem else rv.BatchedMPPI)(B=B3, seeds=[seed_of(i) for i in range(B3)], **kw)
    kw[plan] = eq_plan(rv, b)
    return (rv.CEM if cem else rv.MPPI)(seed=seed_of(b), **kw)


def last_of(ctl, cem, batched=False):
    e = ctl.engine
    return getattr(e, ("cem" if cem else "mppi") + "_last" + ("_batch" if batched else ""))()


@pytest.mark.parametrize("shared", [False, True], ids=["track per problem", "one shared track"])
@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_batch_equals_singles(rv, cem, shared):
    bat = make(rv, cem, None)
    rows = eq_rows(rv, bat, 2, B3)
    tracks = eq_tracks(rows, 4)
    if shared:
        tracks = tracks[:1]
    bat.set_nav(eq_nav(rv, tracks))
    singles = [make(rv, cem, eq_nav(rv, tracks[0 if shared else b], near=tracks), b) for b in range(B3)]
    for t in range(2):
        bat.step(rows[:, t])
        Ub, Jb = last_of(bat, cem, True)
        for b, s in enumerate(singles):
            s.step(rows[b, t])
            assert same(bat.records[b], record_of(s.last)), (t, b)
            for name in (("mean", "std", "elites") if cem else ("nominal",)):
                assert same(getattr(bat, name)[b], getattr(s, name)), (t, b, name)
            for k, v in s.last_stats.items():
                assert same(np.float64(bat.last_stats[k][b]), np.float64(v)), (t, b, k)
            Us, Js = last_of(s, cem)
            assert same(Ub[b], Us) and same(Jb[b], Js), (t, b)
    # the tracks matter: the problems' costs differ from those of a controller without the cost
    plain = make(rv, cem, None, 0)
    plain.step(rows[0, 0]); plain.step(rows[0, 1])
    assert not same(last_of(plain, cem)[1], last_of(singles[0], cem)[1])
    for ctl in [bat, plain] + singles:
        ctl.close()


@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_device_loop_equals_host_steps(rv, cem, feedback):
    """run(rows) of T = 5 against five host steps; the track has 5 rows from origin 2, so the loop starts before the origin
    and its horizon crosses the track's end."""
    T = 5
    dev = make(rv, cem, None, 0)
    rows = eq_rows(rv, dev, T)
    nav = eq_nav(rv, eq_tracks(rows[None], T)[0], origin=2)
    ref = make(rv, cem, nav, 0)
    dev.set_nav(nav)
    res = dev.run(rows, feedback)
    want, _ = host_loop(ref, rows, feedback, cem)
    assert_rows_equal(res, want, ("cem" if cem else "mppi", feedback))
    assert dev.step_count == ref.step_count == T
    assert all(same(a, b) for a, b in zip(last_of(dev, cem), last_of(ref, cem)))
    dev.close(); ref.close()


@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_batched_device_loop_equals_host_steps(rv, cem, feedback):
    T = 5
    dev = make(rv, cem, None)
    rows = eq_rows(rv, dev, T, B3)
    nav = eq_nav(rv, eq_tracks(rows, T), origin=2)
    ref = make(rv, cem, nav)
    dev.set_nav(nav)
    res = dev.run(rows, feedback)
    want = host_loop_batch(ref, rows, feedback, cem)
    assert_rows_equal(res, want, ("cem" if cem else "mppi", feedback))
    assert all(same(a, b) for a, b in zip(last_of(dev, cem, True), last_of(ref, cem, True)))
    dev.close(); ref.close()


@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_step_run_step_along_one_track(rv, cem):
    """step, run(3 rows), step against five steps: the step counter the track is read at advances by 1 and by T."""
    T = 5
    a = make(rv, cem, None, 0)
    rows = eq_rows(rv, a, T)
    nav = eq_nav(rv, eq_tracks(rows[None], T)[0], origin=1)
    b = make(rv, cem, nav, 0)
    a.set_nav(nav)
    want, _ = host_loop(b, rows, False, cem)
    a.step(rows[0])
    assert same(record_of(a.last), want["records"][0])
    res = a.run(rows[1:4])
    assert a.step_count == 4
    assert_rows_equal(res, {k: v[1:4] for k, v in want.items()}, "the run between the steps")
    a.step(rows[4])
    assert same(record_of(a.last), want["records"][4])
    assert same(a.mean if cem else a.nominal, want["plans"][4])
    assert all(same(x, y) for x, y in zip(last_of(a, cem), last_of(b, cem)))
    # without the cost the same five steps give other plans: the track was read
    plain = make(rv, cem, None, 0)
    other, _ = host_loop(plain, rows, False, cem)
    assert not same(other["plans"], want["plans"])
    for ctl in (a, b, plain):
        ctl.close()


# ---- 4. off means off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_cleared_cost_leaves_no_trace(rv, cem, dtype):
    never = make(rv, cem, None, 0, dtype)
    rows = eq_rows(rv, never, 2)
    nav = eq_nav(rv, eq_tracks(rows[None], 2)[0])
    once = make(rv, cem, nav, 0, dtype)
    once.step(rows[0])
    once.set_nav(None)
    once.reset(eq_plan(rv, 0))
    never.step_count = once.step_count
    for t in range(2):
        once.step(rows[t]); never.step(rows[t])
        assert same(record_of(once.last), record_of(never.last)), t
        for name in (("mean", "std", "elites") if cem else ("nominal",)):
            assert same(getattr(once, name), getattr(never, name)), (t, name)
        assert all(same(x, y) for x, y in zip(last_of(once, cem), last_of(never, cem))), t
    res_a, res_b = once.run(rows, True), never.run(rows, True)
    assert_rows_equal(res_a, res_b, "loops after clearing")
    once.close(); never.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_shooting_steps_do_not_read_the_setting(rv, dtype):
    N, K = 8, 256
    state, U, track, spheres = problem(rv, N, K, dtype, seed=2)
    m = rv.default_model()
    out = []
    for with_nav in (False, True):
        with rv.Engine(rv.MPCConfig(N=N, K=K, dtype=dtype)) as e:
            if with_nav:
                e.set_nav_cost(*rv._lib.nav_cost(track(5), spheres=spheres, **WEIGHTS))
            r = e.step(state, U)
            recs = [e.mpc_step_sampled(state, 5, s, m.mean[3:6], m.scale[3:6]).copy() for s in range(3)]
            out.append((record_of(r), np.stack(recs), e.rollout_costs(state, U)))
    for x, y in zip(*out):
        assert same(x, y)


# ---- 5. errors -------------------------------------------------------------------------------------------------------------
def test_errors_keep_the_previous_setting(rv):
    N, K = 6, 64
    state, U, track, spheres = problem(rv, N, K, "f64", seed=3)
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        lib, h = e.lib, e._h
        with pytest.raises(rv.RovmpcError) as ei:                       # nothing set yet
            e.nav_cost(state, U, 0)
        assert ei.value.code == -1 and "no navigation cost" in str(ei.value)
        good, tracks = rv._lib.nav_cost(np.stack([track(4), track(4)]), spheres=spheres[:3], **WEIGHTS)
        e.set_nav_cost(good, tracks)
        C0 = e.nav_cost(state, U, 1)
        assert np.all(C0 > 0)

        def rejected(nav, word):
            rc = lib.rovmpc_set_nav_cost(h, C.byref(nav), tracks.ctypes.data_as(C.c_void_p), 2, 4)
            assert rc == -1 and word in lib.rovmpc_last_error(h).decode(), lib.rovmpc_last_error(h)
            assert same(e.nav_cost(state, U, 1), C0)                    # the previous setting holds

        bad, _ = rv._lib.nav_cost(tracks, **ZERO)
        bad.struct_size += 8
        rejected(bad, "struct_size")
        bad, _ = rv._lib.nav_cost(tracks, **ZERO)
        bad.n_spheres = 9
        rejected(bad, "n_spheres")
        bad, _ = rv._lib.nav_cost(tracks, **ZERO)
        bad.w_du[1] = -1.0
        rejected(bad, "w_du")
        # a batched step with B = 3 against 2 tracks: refused before anything is launched, the setting kept
        p = rv.MPPIParams.make(1, 0.5, defaults(rv, N)[1])
        plans = np.stack([defaults(rv, N)[0]] * 3)
        e.mppi_reset_batch(plans)
        states, seeds = np.tile(state, (3, 1)), [1, 2, 3]
        with pytest.raises(rv.RovmpcError) as ei:
            e.mppi_step_batch(states, seeds, 0, p)
        assert ei.value.code == -1 and "2 tracks" in str(ei.value)
        pc = rv.CEMParams.make(1, 8, 0.0, defaults(rv, N)[1])
        e.cem_reset_batch(plans)
        with pytest.raises(rv.RovmpcError) as ei:
            e.cem_step_batch(states, seeds, 0, pc)
        assert ei.value.code == -1 and "2 tracks" in str(ei.value)
        assert same(e.nav_cost(state, U, 1), C0)
        # the refused step consumed nothing: with one track the step equals that of an engine that never failed
        one, tr1 = rv._lib.nav_cost(track(4), spheres=spheres[:3], **WEIGHTS)
        e.set_nav_cost(one, tr1)
        got = e.mppi_step_batch(states, seeds, 0, p)
        with rv.Engine(rv.MPCConfig(N=N, K=K)) as f:
            f.set_nav_cost(one, tr1)
            f.mppi_reset_batch(plans)
            want = f.mppi_step_batch(states, seeds, 0, p)
        assert all(same(x, y) for x, y in zip(got, want))
        # clearing: the device entry is refused again
        e.set_nav_cost(None)
        with pytest.raises(rv.RovmpcError):
            e.nav_cost(state, U, 0)


def test_unsupported_with_a_communicator(rv):
    """Once rovmpc_comm_init has run the setter and the device entry answer ROVMPC_ERR_UNSUPPORTED (world = 1: no peer is needed)."""
    N, K = 6, 64
    state, U, track, _ = problem(rv, N, K, "f64", seed=4)
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        nav, tr = rv._lib.nav_cost(track(3), **WEIGHTS)
        e.set_nav_cost(nav, tr)
        e.comm_init(e.comm_unique_id(), 0, 1)
        for call in (lambda: e.set_nav_cost(nav, tr), lambda: e.set_nav_cost(None), lambda: e.nav_cost(state, U, 0)):
            with pytest.raises(rv.RovmpcError) as ei:
                call()
            assert ei.value.code == -4
        e.comm_destroy()


# ---- 6. it steers ------------------------------------------------------------------------------------------------------------
def test_mppi_steers_to_a_waypoint(rv):
    """A host-stepped MPPI loop in which the test moves the vehicle by P1 += c u, everything else held: the distance to a
    waypoint 0.1 m away ends smaller than it began.  (The same loop restated on the CPU -- the oracle's sampler and
    rollout, tests/nav_reference.py and the update law -- ends 0.007 m from the waypoint.)"""
    N, K, T = 8, 256, 40
    state, _ = rv.synthetic_problem(K, N)
    way = state[3:6] + 0.1 * np.array([0.8, -0.36, 0.48])
    ctl = rv.MPPI(N=N, K=K, lam=1.0, n_iter=1, seed=11, nominal=np.zeros((N, 3)), lo=(-300.0,) * 3, hi=(300.0,) * 3,
                  nav=rv.NavCost(way[None], w_pos=1e4))
    c, d0 = c_of(ctl.cfg), float(np.linalg.norm(state[3:6] - way))
    for t in range(T):
        u = ctl.step(state)
        state = state.copy()
        state[3:6] += c * u
        print(f"step {t}: distance {np.linalg.norm(state[3:6] - way):.6f} m")
    ctl.close()
    assert np.linalg.norm(state[3:6] - way) < d0
