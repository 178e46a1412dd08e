"""The tether keep-out cost of MPPI and CEM on the GPU (rovmpc_set_tether_cost, rovmpc_tether_cost_device; law in
include/rovmpc.h): the term against the 50-digit reference of tests/tether_reference.py within the measured margin times
each node's conditioning scale, its determinism, w = 0 leaving every bit (the proof that handing the rollout a trajectory
buffer changes nothing it returns), the MPPI and CEM steps reading J' bit for bit, the batch and device-loop equivalences
with a navigation and a tether cost on, hygiene, and a closed loop that steers the cable off a sphere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from mpmath import mp, mpf

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tether_reference as tr  # noqa: E402
from plan_controller_helpers import colmax, defaults, rv  # noqa: E402,F401
from plan_loop_helpers import assert_rows_equal, host_loop, host_loop_batch, record_of, same  # noqa: E402
from test_cem_host import cem_elites, cem_update_ref  # noqa: E402
from test_mppi_host import mppi_update_ref  # noqa: E402

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}


def scene_engine(rv, sc, dtype, **kw):
    return rv.Engine(rv.MPCConfig(N=sc.N, K=sc.K, dtype=dtype, n_shape_pts=sc.M, c_lo=tr.BRACKET[0], c_hi=tr.BRACKET[1], L=tr.L_WS,
                                  frame="ENU" if sc.up > 0 else "NED", **kw))


def setting(rv, spheres, w=tr.W, margin=tr.MARGIN):
    return rv._lib.tether_cost(spheres, w, margin)


# ---- 1. the term against the reference ------------------------------------------------------------------------------------
CASES = [(N, K, M, 1.0) for N, K, M in tr.SHAPES] + [tr.FRAMES_AT + (-1.0,)]


@pytest.mark.parametrize("N,K,M,up", CASES, ids=lambda v: str(v))
def test_term_against_reference(rv, N, K, M, up):
    """D within m s, C within sum w (2 pen delta + delta^2), J' within that plus one ulp of T, with 1, 3 and 8 spheres in fp64
    and fp32 (the scene's values are exact in both); a non-finite J is kept bit for bit."""
    sc, ref8 = tr.scene_reference(N, K, M, up)
    assert tr.C_STEP == rv.MPCConfig().v_scale * rv.MPCConfig().dt
    rng = np.random.default_rng(N + K)
    for dtype in ("f64", "f32"):
        with scene_engine(rv, sc, dtype) as e:
            for n_sph in (1, 3, 8):
                ref = tr.prefix(ref8, n_sph)
                sph = sc.spheres[:n_sph]
                e.set_tether_cost(setting(rv, sph))
                Cg, Dg = e.tether_cost(sc.state, sc.U, sc.traj)
                bD, bC = tr.bounds(ref, sc.state, sph, tr.W)
                eC, eD = tr.errors(Cg, Dg, ref)
                rD, rC = tr.ratios(Cg, Dg, ref, sc.state, sph, tr.W)
                print(f"N {N} K {K} M {M} up {up:+.0f} {dtype} {n_sph} spheres: largest error / scale: D {rD:.3g}, C {rC:.3g} (m = {tr.M_TETHER})")
                assert np.all(eD <= bD), (dtype, n_sph, rD)
                assert np.all(eC <= bC), (dtype, n_sph, rC)
                # the in-place form, with an inf and a NaN planted
                J = rng.uniform(0.05, 5.0, K).astype(NP[dtype])
                if K >= 5:
                    J[1], J[K - 2] = np.inf, np.nan
                C2, D2, Jp = e.tether_cost(sc.state, sc.U, sc.traj, J=J)
                assert same(C2, Cg) and same(D2, Dg)
                excess = tr.check_J(Jp, J, ref, bC, NP[dtype])
                print(f"    largest |J' - (J + C_ref)| over its allowance: {excess:.3g}")
                assert excess <= 1.0, (dtype, n_sph, excess)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nan_angle_gives_inf_and_nan_at_that_node_only(rv, dtype):
    N, K, M = 11, 67, 16
    sc = tr.scene(N, K, M)
    with scene_engine(rv, sc, dtype) as e:
        e.set_tether_cost(setting(rv, sc.spheres[:3]))
        C0, D0 = e.tether_cost(sc.state, sc.U, sc.traj)
        assert np.all(np.isfinite(C0)) and np.all(np.isfinite(D0))
        traj = sc.traj.copy()
        planted = [(0, 1, 0), (5, N, 0), (K - 1, 4, 1), (33, 7, 0)]            # (row, node, theta or gamma)
        for i, (k, n, a) in enumerate(planted):
            traj[k, n, a] = np.nan if i != 3 else np.inf
        traj[9, 0, 0] = np.nan                                                 # node 0 is not read
        J = np.linspace(0.5, 2.0, K).astype(NP[dtype])
        C1, D1, J1 = e.tether_cost(sc.state, sc.U, traj, J=J)
        rows = [k for k, _, _ in planted]
        want_D = D0.copy()
        for k, n, _ in planted:
            want_D[k, n - 1] = np.nan
        assert np.array_equal(np.isnan(D1), np.isnan(want_D))
        assert same(np.where(np.isnan(want_D), 0.0, D1), np.where(np.isnan(want_D), 0.0, D0))
        assert np.all(C1[rows] == np.inf) and np.all(J1[rows] == np.inf)
        others = np.setdiff1d(np.arange(K), rows)
        assert same(C1[others], C0[others])


# ---- 2. determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rows_give_the_same_bits_wherever_they_are(rv, dtype):
    """The rows of the (11, 67, 16) scene at other places k (another tile, another place in it) and in another K, through the
    device entry; that a batch's problems give their single controllers' bits is test_batch_equals_singles below."""
    N, K, M = 11, 67, 16
    sc = tr.scene(N, K, M)
    sph = sc.spheres[:3]
    with scene_engine(rv, sc, dtype) as e:
        e.set_tether_cost(setting(rv, sph))
        C0, D0 = e.tether_cost(sc.state, sc.U, sc.traj)
    perm = np.random.default_rng(3).permutation(K)
    K2 = 2 * K + 3                              # no multiple of the tile; the rows once permuted, once in order, three more
    idx = np.concatenate([perm, np.arange(K), [5, 5, 0]])
    big = sc._replace(K=K2)
    with scene_engine(rv, big, dtype) as e:
        e.set_tether_cost(setting(rv, sph))
        C1, D1 = e.tether_cost(sc.state, sc.U[idx], sc.traj[idx])
    assert same(C1, C0[idx]) and same(D1, D0[idx])
    one = sc._replace(K=1)
    with scene_engine(rv, one, dtype) as e:
        e.set_tether_cost(setting(rv, sph))
        for k in (0, 13, K - 1):
            C2, D2 = e.tether_cost(sc.state, sc.U[k:k + 1], sc.traj[k:k + 1])
            assert same(C2, C0[k:k + 1]) and same(D2, D0[k:k + 1])


# ---- shared by the controller tests ---------------------------------------------------------------------------------------
EQ = dict(N=6, K=256)
B3 = 3


def eq_rows(rv, ctl, T, B=None):
    from rovmpc.closed_loop import closed_loop_inputs
    if B is None:
        return closed_loop_inputs(ctl.engine, 12, T)[0]
    return np.ascontiguousarray(closed_loop_inputs(ctl.engine, 12, B * T)[0].reshape(B, T, 16))


def cable_spheres(rows):
    """Two spheres the cables of the measured rows (16,) pass through: centred a few centimetres beside the middle of the
    connection vector of the first row, and a quarter of the way along that of the last."""
    rows = np.asarray(rows).reshape(-1, 16)
    a, b = rows[0], rows[-1]
    return np.array([np.concatenate([a[0:3] + 0.5 * (a[3:6] - a[0:3]) + [0.03, -0.02, 0.0], [0.9]]),
                     np.concatenate([b[0:3] + 0.25 * (b[3:6] - b[0:3]) + [0.0, 0.02, 0.05], [0.6]])])


def eq_tether(rv, rows, w=50.0):
    return rv.TetherCost(cable_spheres(rows), w, margin=0.02)


def eq_nav(rv, rows):
    rows = np.asarray(rows).reshape(-1, 16)
    track = rows[:4, 3:6] + 0.003
    sph = np.concatenate([track[:2] + 0.002, [[0.004], [0.006]][:len(track[:2])]], axis=1)
    return rv.NavCost(track, w_pos=(2e3, 1e3, 3e3), w_term=5e3, w_du=(1e-4, 0.0, 2e-4), w_sphere=1e4, spheres=sph)


def seed_of(b):
    return 1000003 * (b + 1) + 17


def eq_plan(rv, b):
    mean, std = defaults(rv, EQ["N"])
    return mean + 0.05 * std * np.random.default_rng(500 + b).standard_normal((EQ["N"], 3))


def make(rv, cem, b=None, dtype="f64", n_iter=2, nav=None, tether=None, **cfg):
    """A single controller of problem b, or (b None) the batched one of B3 problems."""
    kw = dict(dtype=dtype, n_iter=n_iter, nav=nav, tether=tether, **EQ)
    kw.update(cfg)
    N = kw["N"]
    if cem:
        _, std = defaults(rv, N)
        kw.update(n_elite=16, alpha=0.15, std_min=0.02 * std)
    else:
        kw.update(lam=0.5)
    plan = "mean" if cem else "nominal"
    if N == EQ["N"]:
        kw[plan] = np.stack([eq_plan(rv, i) for i in range(B3)]) if b is None else eq_plan(rv, b)
    if b is None:
        return (rv.BatchedCEM if cem else rv.BatchedMPPI)(B=B3, seeds=[seed_of(i) for i in range(B3)], **kw)
    return (rv.CEM if cem else rv.MPPI)(seed=seed_of(b), **kw)


def last_of(ctl, cem, batched=False):
    e = ctl.engine
    return getattr(e, ("cem" if cem else "mppi") + "_last" + ("_batch" if batched else ""))()


def plan_state(ctl, cem):
    return [getattr(ctl, name) for name in (("mean", "std", "elites") if cem else ("nominal",))]


# ---- 3. w = 0 leaves every bit ------------------------------------------------------------------------------------------------
def check_w0(rv, cem, dtype, **cfg):
    kw = dict(N=8, K=256, **cfg)
    plain = make(rv, cem, 0, dtype, **kw)
    rows = eq_rows(rv, plain, 3)
    zero = make(rv, cem, 0, dtype, tether=eq_tether(rv, rows, w=0.0), **kw)
    for t in range(3):
        plain.step(rows[t]); zero.step(rows[t])
        assert same(record_of(zero.last), record_of(plain.last)), t
        for x, y in zip(plan_state(zero, cem), plan_state(plain, cem)):
            assert same(x, y), t
        for k, v in plain.last_stats.items():
            assert same(np.float64(zero.last_stats[k]), np.float64(v)), (t, k)
        assert all(same(x, y) for x, y in zip(last_of(zero, cem), last_of(plain, cem))), t
    path = zero.engine.model_path
    plain.close(); zero.close()
    return path


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_zero_weight_leaves_every_bit(rv, cem, dtype):
    assert check_w0(rv, cem, dtype) == "builtin"


@pytest.mark.parametrize("path,cfg", [("jit", dict(no_builtin=True)), ("interpreter", dict(force_interpreter=True))])
def test_zero_weight_leaves_every_bit_on_the_other_model_paths(rv, path, cfg):
    assert check_w0(rv, False, "f64", **cfg) == path


# ---- 4. the step reads it ------------------------------------------------------------------------------------------------------
def expected_step_costs(rv, ctl, U, state, step, dtype, nav, tether, **cfg):
    """J' of the law for the reported candidates: rollout costs and trajectories of a plain engine (on the model path `cfg`
    names), the navigation term, then the device entry's tether term applied in place.  Returns (J', J, C)."""
    with rv.Engine(rv.MPCConfig(N=ctl.cfg.N, K=ctl.cfg.K, dtype=dtype, **cfg)) as plain:
        J, traj = plain.rollout_costs(state, U, return_traj=True)
        J1 = J
        if nav is not None:
            plain.set_nav_cost(nav.c_nav, nav.tracks)
            _, J1 = plain.nav_cost(state, U, step, J=J)
        plain.set_tether_cost(tether.c_tether)
        Ct, _, J2 = plain.tether_cost(state, U, traj, J=J1)
    return J2, J, Ct


@pytest.mark.parametrize("with_nav", [False, True], ids=["tether", "nav+tether"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mppi_step_reads_the_tether_cost(rv, dtype, with_nav):
    N, K, lam, step = 8, 256, 1.0, 3
    state, _ = rv.synthetic_problem(1, N)
    nav, tether = (eq_nav(rv, state) if with_nav else None), eq_tether(rv, state)
    ctl = rv.MPPI(N=N, K=K, dtype=dtype, lam=lam, n_iter=2, seed=9, nav=nav, tether=tether)
    ctl.step_count = step
    u = ctl.step(state)
    U, Jp = ctl.engine.mppi_last()
    want, J, Ct = expected_step_costs(rv, ctl, U, state, step, dtype, nav, tether)
    assert same(Jp, want)
    fin = np.isfinite(J)
    assert fin.sum() >= K // 2 and np.all(Ct[fin] > 0) and not same(Jp, J)
    nu_ref, st_ref = mppi_update_ref(Jp, U, lam, np.zeros((N, 3)))
    assert np.abs(ctl.nominal - nu_ref).max() <= 1e-12 * np.abs(U).max()
    assert np.array_equal(u, ctl.nominal[0])
    st = ctl.last_stats
    assert st["rho"] == Jp[np.isfinite(Jp)].min() and st["J0"] == Jp[0]
    assert st["eta"] == pytest.approx(st_ref[1], rel=1e-12) and st["ess"] == pytest.approx(st_ref[2], rel=1e-12)
    ctl.close()


@pytest.mark.parametrize("path,cfg", [("jit", dict(no_builtin=True)), ("interpreter", dict(force_interpreter=True))])
def test_mppi_step_reads_the_tether_cost_on_the_other_model_paths(rv, path, cfg):
    """The trajectory buffer the hiprtc and interpreter kernels fill holds the angles the law names: J' of a step on that path
    is, bit for bit, the device entry's term on the trajectories rovmpc_rollout_costs returns on the same path, and those
    are the compiled-in path's angles to rounding, so the costs are not those of some other finite buffer."""
    N, K, lam, step = 8, 256, 1.0, 3
    state, _ = rv.synthetic_problem(1, N)
    tether = eq_tether(rv, state)
    ctl = rv.MPPI(N=N, K=K, lam=lam, n_iter=2, seed=9, tether=tether, **cfg)
    assert ctl.engine.model_path == path
    ctl.step_count = step
    ctl.step(state)
    U, Jp = ctl.engine.mppi_last()
    want, J, Ct = expected_step_costs(rv, ctl, U, state, step, "f64", None, tether, **cfg)
    assert same(Jp, want)
    fin = np.isfinite(J)
    assert fin.sum() >= K // 2 and np.all(Ct[fin] > 0) and not same(Jp, J)
    # against the compiled-in path on the same candidates.  The project's parity rule between model paths is 1e-5 relative
    # on the angles (smoke(), the parity tests): angles of at most 0.1 rad then differ by 1e-6 rad, the points of a 3 m cable
    # under two angles by at most 6e-6 m, and C = w sum pen^2 with penetrations of some 0.3 m and more into spheres of 0.6
    # and 0.9 m by at most 2 * 6e-6 / 0.3 = 4e-5 relative; 1e-4 is asked.  Another buffer's angles would move C by order 1.
    _, _, Cb = expected_step_costs(rv, ctl, U, state, step, "f64", None, tether)
    assert np.all(np.abs(Ct[fin] - Cb[fin]) <= 1e-4 * np.abs(Cb[fin]))
    nu_ref, _ = mppi_update_ref(Jp, U, lam, np.zeros((N, 3)))
    assert np.abs(ctl.nominal - nu_ref).max() <= 1e-12 * np.abs(U).max()
    ctl.close()


@pytest.mark.parametrize("with_nav", [False, True], ids=["tether", "nav+tether"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cem_step_reads_the_tether_cost(rv, dtype, with_nav):
    N, K, E, step = 8, 256, 16, 3
    _, std = defaults(rv, N)
    state, _ = rv.synthetic_problem(1, N)
    nav, tether = (eq_nav(rv, state) if with_nav else None), eq_tether(rv, state)
    ctl = rv.CEM(N=N, K=K, dtype=dtype, n_elite=E, n_iter=2, alpha=0.0, seed=9, nav=nav, tether=tether)
    ctl.step_count = step
    ctl.step(state)
    U, Jp = ctl.engine.cem_last()
    want, J, Ct = expected_step_costs(rv, ctl, U, state, step, dtype, nav, tether)
    assert same(Jp, want)
    fin = np.isfinite(J)
    assert fin.sum() >= K // 2 and np.all(Ct[fin] > 0) and not same(Jp, J)
    assert np.array_equal(ctl.elites, cem_elites(Jp, E))
    mu_r, sg_r, el_r, st_r = cem_update_ref(Jp, U, E, 0.0, (0.0, 0.0, 0.0), np.zeros((N, 3)), np.tile(std, (N, 1)))
    cm = colmax(U, (N, 3))
    assert np.all(np.abs(ctl.mean - mu_r) <= 1e-12 * cm) and np.all(np.abs(ctl.std - sg_r) <= 1e-12 * cm)
    st = ctl.last_stats
    assert [st["J_best"], st["J_worst_elite"], st["n_finite"], st["J0"]] == list(st_r)
    ctl.close()


# ---- 5. the equivalences, bit for bit, with a navigation and a tether cost on ---------------------------------------------
@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_batch_equals_singles(rv, cem):
    bat = make(rv, cem)
    rows = eq_rows(rv, bat, 2, B3)
    nav, tether = eq_nav(rv, rows[0]), eq_tether(rv, rows[:, 0])
    bat.set_nav(nav); bat.set_tether(tether)
    singles = [make(rv, cem, b, nav=nav, tether=tether) for b in range(B3)]
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
    # the tether cost matters: with the navigation cost alone the costs differ
    other = make(rv, cem, 0, nav=nav)
    other.step(rows[0, 0]); other.step(rows[0, 1])
    assert not same(last_of(other, cem)[1], last_of(singles[0], cem)[1])
    for ctl in [bat, other] + singles:
        ctl.close()


@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_device_loop_equals_host_steps(rv, cem, feedback):
    T = 4
    dev = make(rv, cem, 0)
    rows = eq_rows(rv, dev, T)
    nav, tether = eq_nav(rv, rows), eq_tether(rv, rows)
    ref = make(rv, cem, 0, nav=nav, tether=tether)
    dev.set_nav(nav); dev.set_tether(tether)
    res = dev.run(rows, feedback)
    want, _ = host_loop(ref, rows, feedback, cem)
    assert_rows_equal(res, want, ("cem" if cem else "mppi", feedback))
    assert all(same(a, b) for a, b in zip(last_of(dev, cem), last_of(ref, cem)))
    dev.close(); ref.close()


@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_batched_device_loop_equals_host_steps(rv, cem, feedback):
    T = 4
    dev = make(rv, cem)
    rows = eq_rows(rv, dev, T, B3)
    nav, tether = eq_nav(rv, rows[0]), eq_tether(rv, rows[:, 0])
    ref = make(rv, cem, nav=nav, tether=tether)
    dev.set_nav(nav); dev.set_tether(tether)
    res = dev.run(rows, feedback)
    want = host_loop_batch(ref, rows, feedback, cem)
    assert_rows_equal(res, want, ("cem" if cem else "mppi", feedback))
    assert all(same(a, b) for a, b in zip(last_of(dev, cem, True), last_of(ref, cem, True)))
    dev.close(); ref.close()


# ---- 6. hygiene ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_cleared_cost_leaves_no_trace(rv, cem, dtype):
    never = make(rv, cem, 0, dtype)
    rows = eq_rows(rv, never, 2)
    once = make(rv, cem, 0, dtype, tether=eq_tether(rv, rows))
    once.step(rows[0])
    once.set_tether(None)
    once.reset(eq_plan(rv, 0))
    never.step_count = once.step_count
    for t in range(2):
        once.step(rows[t]); never.step(rows[t])
        assert same(record_of(once.last), record_of(never.last)), t
        for x, y in zip(plan_state(once, cem), plan_state(never, cem)):
            assert same(x, y), t
        assert all(same(x, y) for x, y in zip(last_of(once, cem), last_of(never, cem))), t
    assert_rows_equal(once.run(rows, True), never.run(rows, True), "loops after clearing")
    once.close(); never.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_shooting_steps_do_not_read_the_setting(rv, dtype):
    N, K = 8, 256
    state, U = rv.synthetic_problem(K, N, dtype=NP[dtype])
    m = rv.default_model()
    out = []
    for with_cost in (False, True):
        with rv.Engine(rv.MPCConfig(N=N, K=K, dtype=dtype)) as e:
            if with_cost:
                e.set_tether_cost(setting(rv, cable_spheres(state), 50.0, 0.02))
            r = e.step(state, U)
            recs = [e.mpc_step_sampled(state, 5, s, m.mean[3:6], m.scale[3:6]).copy() for s in range(3)]
            out.append((record_of(r), np.stack(recs), e.rollout_costs(state, U)))
    for x, y in zip(*out):
        assert same(x, y)


def test_errors_keep_the_previous_setting(rv):
    N, K = 6, 64
    state, U = rv.synthetic_problem(K, N)
    sph = cable_spheres(state)
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        lib, h = e.lib, e._h
        _, traj = e.rollout_costs(state, U, return_traj=True)
        with pytest.raises(rv.RovmpcError) as ei:                       # nothing set yet
            e.tether_cost(state, U, traj)
        assert ei.value.code == -1 and "no tether cost" in str(ei.value)
        e.set_tether_cost(setting(rv, sph, 50.0, 0.02))
        C0, D0 = e.tether_cost(state, U, traj)
        assert np.all(C0 > 0)

        def rejected(change, word):
            bad = setting(rv, sph, 1.0, 0.0)
            change(bad)
            rc = lib.rovmpc_set_tether_cost(h, C.byref(bad))
            assert rc == -1 and word in lib.rovmpc_last_error(h).decode(), lib.rovmpc_last_error(h)
            got = e.tether_cost(state, U, traj)                         # the previous setting holds
            assert same(got[0], C0) and same(got[1], D0)

        rejected(lambda t: setattr(t, "struct_size", t.struct_size + 8), "struct_size")
        rejected(lambda t: setattr(t, "n_spheres", 0), "n_spheres")
        rejected(lambda t: setattr(t, "n_spheres", 9), "n_spheres")
        rejected(lambda t: setattr(t, "w", -1.0), "w must")
        rejected(lambda t: setattr(t, "w", np.inf), "w must")
        rejected(lambda t: setattr(t, "margin", -0.01), "margin")
        rejected(lambda t: setattr(t, "margin", np.nan), "margin")
        rejected(lambda t: t.spheres[1].__setitem__(3, -0.5), "sphere 1")
        rejected(lambda t: t.spheres[0].__setitem__(1, np.nan), "sphere 0")
        # null inputs of the device entry
        rc = lib.rovmpc_tether_cost_device(h, None, None, None, None, None, None, None)
        assert rc == -1 and "null pointer" in lib.rovmpc_last_error(h).decode()
        e.set_tether_cost(None)
        with pytest.raises(rv.RovmpcError):
            e.tether_cost(state, U, traj)


def test_unsupported_with_a_communicator(rv):
    """Once rovmpc_comm_init has run the setter and the device entry answer ROVMPC_ERR_UNSUPPORTED (world = 1: no peer is needed)."""
    N, K = 6, 64
    state, U = rv.synthetic_problem(K, N)
    with rv.Engine(rv.MPCConfig(N=N, K=K)) as e:
        t = setting(rv, cable_spheres(state), 50.0, 0.02)
        e.set_tether_cost(t)
        traj = np.zeros((K, N + 1, 2))
        e.comm_init(e.comm_unique_id(), 0, 1)
        for call in (lambda: e.set_tether_cost(t), lambda: e.set_tether_cost(None), lambda: e.tether_cost(state, U, traj)):
            with pytest.raises(rv.RovmpcError) as ei:
                call()
            assert ei.value.code == -4
        e.comm_destroy()


# ---- 7. it steers the cable ------------------------------------------------------------------------------------------------
STEER_SPHERE = (0.0404, -0.4838, -1.1986, 0.10)


def cable_clearance(cfg, state, sphere):
    """Clearance of the cable of `state` (its P0, P1, theta, gamma) from the sphere at 50 digits, as a float."""
    with mp.workdps(tr.DPS):
        A = [mpf(float(x)) for x in state[0:3]]
        P = [mpf(float(x)) for x in state[3:6]]
        pts, _, _, _ = tr.node_points(A, P, float(state[12]), float(state[13]), mpf(cfg.L), cfg.n_shape_pts, mpf(1), mpf(cfg.c_lo), mpf(cfg.c_hi))
        return float(tr.cable_distance(pts, [mpf(sphere[i]) - A[i] for i in range(3)]) - mpf(sphere[3]))


def test_mppi_steers_the_cable_off_a_sphere(rv):
    """Two host-stepped MPPI loops of 20 steps from the same seed in which the test moves the vehicle by P1 += c u, everything
    else held.  A sphere of 0.1 m sits beside the middle of the initial cable and overlaps it by 3 cm.  The loop with the
    tether cost ends with a strictly larger cable clearance than the loop without.  (The same two loops restated on the CPU
    -- NumPy draws, the oracle's rollout, tether_reference.tether_np and the update law -- end at +0.004 m with the cost and
    -0.030 m without.)"""
    N, K, T = 8, 256, 20
    state0, _ = rv.synthetic_problem(K, N)
    final = []
    for with_cost in (True, False):
        ctl = rv.MPPI(N=N, K=K, lam=1.0, n_iter=1, seed=11, nominal=np.zeros((N, 3)), lo=(-300.0,) * 3, hi=(300.0,) * 3,
                      tether=rv.TetherCost([STEER_SPHERE], 1e4) if with_cost else None)
        c, state = ctl.cfg.v_scale * ctl.cfg.dt, state0.copy()
        if with_cost:
            d0 = cable_clearance(ctl.cfg, state, STEER_SPHERE)
            assert -0.04 < d0 < -0.02, d0
        for t in range(T):
            u = ctl.step(state)
            state = state.copy()
            state[3:6] += c * u
        final.append(cable_clearance(ctl.cfg, state, STEER_SPHERE))
        print(f"tether cost {'on' if with_cost else 'off'}: cable clearance {d0:+.5f} m -> {final[-1]:+.5f} m, P1 moved {state[3:6] - state0[3:6]}")
        ctl.close()
    assert final[0] > final[1]
