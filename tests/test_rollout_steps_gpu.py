"""The (theta, gamma) trajectory that rollout_kernel* integrates, step by step against the 50-digit one-step reference of
tests/rollout_reference.py: every decided step of every candidate within M_STEP x the step's own scale, restarted from the
kernel's own nodes -- so dt = 0.05, long horizons and operating points far from the scaler mean are testable -- and the
w_theta, w_gamma, w_u terms and the default-weight J read off the returned trajectory.  Every case is one
rollout_costs(state, U, return_traj=True) call (and a step() where the record is checked); each test prints its largest
ratio before it asserts."""
import functools

import numpy as np
import pytest

import rollout_reference as rr
from rollout_gpu_helpers import oracle_cfg, oracle_model, rand_rtab, record_is_the_best_row, rollout

pytestmark = pytest.mark.gpu

ZERO_W = dict(w_theta=0.0, w_gamma=0.0, w_u=0.0, w_T=0.0, w_taut=0.0, w_floor=0.0)


@pytest.fixture(scope="module")
def rv():
    import rovmpc
    return rovmpc


@pytest.fixture(scope="module")
def orc():
    from oracle import rovmpc_oracle
    return rovmpc_oracle


def check_steps(rv, orc, cfg, model, state, U, Rtab=None, what="", limit=None, path=None, skip=(), with_step=False):
    """One rollout_costs call, every decided step of every candidate (but those in `skip`) against the reference; with_step:
    step()'s record is row arg-min J of that call, bit for bit."""
    U, J, traj, res = rollout(rv, cfg, model, state, U, Rtab, with_step=with_step, path=path)
    rt, rg, dth = rr.step_ratios(oracle_cfg(orc, cfg), oracle_model(orc, model), state, U, traj, cfg.dtype, Rtab, limit=limit)
    keep = np.array([k not in skip for k in range(len(U))])
    w = rr.worst(rt[keep], rg[keep])
    print("%s %s: largest ratio %.3f of M_STEP %.2f (theta %.3f, gamma %.3f; decided %d + %d of %d steps)"
          % (what, cfg.dtype, w, rr.M_STEP, rr.worst(rt[keep], rt[keep]), rr.worst(rg[keep], rg[keep]), (~np.isnan(rt[keep])).sum(),
             (~np.isnan(rg[keep])).sum(), rt[keep].size))
    assert (~np.isnan(rt[keep])).any() and (~np.isnan(rg[keep])).any(), what
    assert w <= rr.M_STEP, (what, w)
    if with_step:
        record_is_the_best_row(res, U, J, traj)
    return U, J, traj, rt, rg


# ---- sweep -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sweep_row(i, dtype):
    import rovmpc as rv
    from oracle import rovmpc_oracle as orc
    row = rr.table()[i]
    cfg = rv.MPCConfig(N=20, K=rr.K_TABLE, dtype=dtype)
    return check_steps(rv, orc, cfg, rv.default_model(), row.state, row.U, what="sweep " + row.tag, path="builtin",
                       skip=(rr.NAN_CANDIDATE,) if i == rr.NAN_ROW else ())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("i", range(len(rr.table())))
def test_sweep_of_the_workspace(i, dtype):
    """The whole table on the compiled-in rows: composed velocity transform, RK4, interpolated delay slot, N = 20."""
    _sweep_row(i, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_specials_of_the_sweep(rv, orc, dtype):
    """The NaN candidate has NaN theta nodes (gamma's equation reads no control: its nodes are the oracle's, finite) and J = +inf
    while its workgroup stays within bound; the workgroup of the 3e10 control is within bound on the checked sine; duplicate
    candidates return the same bits."""
    U, J, traj, rt, rg = _sweep_row(rr.NAN_ROW, dtype)
    c = rr.NAN_CANDIDATE
    assert np.isnan(traj[c, 1:, 0]).all() and np.isposinf(J[c])
    row = rr.table()[rr.NAN_ROW]
    _, trajo, _ = orc.rollout_vec(oracle_cfg(orc, rv.MPCConfig(N=20, K=rr.K_TABLE, dtype=dtype)), oracle_model(orc, rv.default_model()),
                                  orc.MPCState.from_array(row.state), U.astype(np.float64))
    assert np.array_equal(np.isnan(traj), np.isnan(trajo))
    others = [k for k in range(16) if k != c]
    assert np.isfinite(J[others]).all() and not np.isnan(rt[others]).all()
    U, J, traj, rt, rg = _sweep_row(rr.HUGE_ROW, dtype)
    assert np.isfinite(traj[:16]).all() and not np.isnan(rt[:16]).all() and rr.worst(rt[:16], rg[:16]) <= rr.M_STEP
    for i in range(len(rr.table())):
        U, J, traj, _, _ = _sweep_row(i, dtype)
        assert np.array_equal(U[0], U[-1])
        assert J[0] == J[-1] and np.array_equal(traj[0], traj[-1]), rr.table()[i].tag


# ---- modes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("prev_mode,integrator", [(0, 0), (1, 0), (0, 1)])
@pytest.mark.parametrize("vt_mode", [0, 1, 2])
@pytest.mark.parametrize("op", [2, 4])
def test_modes_away_from_the_scaler_mean(rv, orc, op, vt_mode, prev_mode, integrator, dtype):
    """(0.6, -0.6) -- steps around 2^-6, lanes mix -- and (1.5, 0.3) -- every step a big one --, N = 18 so that step 16
    re-anchors, in every velocity transform, with the held delay slot and with Euler."""
    row = rr.table(18)[op]
    cfg = rv.MPCConfig(N=18, K=8, vt_mode=vt_mode, prev_mode=prev_mode, integrator=integrator, dtype=dtype)
    check_steps(rv, orc, cfg, rv.default_model(), row.state, row.U[:8], rand_rtab(18) if vt_mode == 2 else None,
                what="modes vt=%d prev=%d integ=%d %s" % (vt_mode, prev_mode, integrator, row.tag), path="builtin")


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,dtype,dt", [(1, 1, "f64", 1 / 60), (7, 67, "f64", 1 / 60), (7, 67, "f32", 1 / 60), (21, 5, "f64", 1 / 60),
                                          (21, 5, "f32", 1 / 60), (50, 19, "f32", 1 / 60), (150, 8, "f64", 1 / 240), (150, 8, "f32", 1 / 240)])
def test_shapes(rv, orc, N, K, dtype, dt):
    """A single candidate and step; odd sizes over several workgroups; the first horizon with 3N + 2 > 64 items on the gamma
    wave; the literal-50 instance of fp32; a long horizon at the data rate of 240 Hz.  step() runs the plain single-problem
    instances (the literal horizons among them): its record is the checked call's best row, bit for bit."""
    row = rr.table(N)[2]
    U = rr.controls(N, K, seed=N)
    check_steps(rv, orc, rv.MPCConfig(N=N, K=K, dtype=dtype, dt=dt), rv.default_model(), row.state, U, what="shape N=%d K=%d" % (N, K), path="builtin",
                with_step=True)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_candidates_per_block_does_not_change_the_bits(rv, orc, dtype):
    row = rr.table()[4]
    out = []
    for ck in (1, 16):
        out.append(rollout(rv, rv.MPCConfig(N=20, K=rr.K_TABLE, dtype=dtype, candidates_per_block=ck), rv.default_model(), row.state, row.U))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    check_steps(rv, orc, rv.MPCConfig(N=20, K=rr.K_TABLE, dtype=dtype, candidates_per_block=1), rv.default_model(), row.state, row.U,
                what="one candidate per workgroup " + row.tag)


# ---- model paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,path,dtype", [(dict(force_interpreter=True), "interpreter", "f64"), (dict(force_interpreter=True), "interpreter", "f32"),
                                           (dict(no_builtin=True), "jit", "f64"), (dict(no_builtin=True), "jit", "f32")])
def test_chosen_rows_on_the_interpreter_and_hiprtc(rv, orc, kw, path, dtype):
    for op in (2, 4):
        row = rr.table(12)[op]
        check_steps(rv, orc, rv.MPCConfig(N=12, K=rr.K_TABLE, dtype=dtype, **kw), rv.default_model(), row.state, row.U,
                    what="chosen rows, %s, %s" % (path, row.tag), path=path)


@pytest.mark.parametrize("jit", [True, False])
def test_rows_whose_gamma_slope_depends_on_the_candidate(rv, orc, jit):
    """Rows (5, 9): dgamma/dt reads x3, so the gamma path is no longer one table per workgroup."""
    model = rv.default_model(5, 9)
    for op in (2, 4):
        row = rr.table(12)[op]
        check_steps(rv, orc, rv.MPCConfig(N=12, K=rr.K_TABLE, jit=jit), model, row.state, row.U, what="rows (5, 9), jit=%s, %s" % (jit, row.tag),
                    path="jit" if jit else "interpreter")


@pytest.mark.parametrize("jit", [True, False])
def test_generation2_map(rv, orc, jit):
    model = rv.generation2_model()
    for op in (2, 4):
        row = rr.table(12)[op]
        check_steps(rv, orc, rv.MPCConfig(N=12, K=rr.K_TABLE, jit=jit, feature_map=rv.FEATURES_GEN2), model, row.state, row.U,
                    what="generation 2, jit=%s, %s" % (jit, row.tag), path="jit" if jit else "interpreter")


# ---- dt = 0.05 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kw,path", [(dict(), "builtin"), (dict(no_builtin=True), "jit")])
def test_the_step_of_survey_and_verdict(rv, orc, kw, path, dtype):
    """dt = 0.05 s, where the gamma recurrence amplifies rounding by 1e20 over the horizon (|gamma| = 1.4e5 at node 10 of the
    oracle, 1.4e10 at node 15): compared step by step from the kernel's own nodes while |theta_n| and |gamma_n| are below 2^20.
    A step counts as compared when theta or gamma of it is held to the bound; in fp64 both are, on 8 steps or more.  In fp32
    theta's steps are undecided from |gamma| ~ 60 on by the rule of rollout_reference (scale > 1e-3 of the increment): dtheta/dt
    reads sin(x17), x17 = gamma_prev / 0.0173 carries 2 eps32 |x17| from its scaling, so the scale of theta's step is
    h 0.048 * 1.4e-5 |gamma| against an increment of about h 0.048 -- measured: 7 to 9 steps per candidate from the synthetic
    state, 6 from (0.6, -0.6), where gamma's own steps are compared on 10 and 8."""
    s0, _ = rv.synthetic_problem(1, 20)
    for state, tag in ((s0, "synthetic state"), (rr.table()[2].state, rr.table()[2].tag)):
        U = rr.controls(20, seed=50)
        _, J, traj, rt, rg = check_steps(rv, orc, rv.MPCConfig(N=20, K=rr.K_TABLE, dt=0.05, dtype=dtype, **kw), rv.default_model(), state, U,
                                         what="dt=0.05 %s %s" % (path, tag), limit=2.0 ** 20, path=path)
        n_th, n_ga = (~np.isnan(rt)).sum(axis=1), (~np.isnan(rg)).sum(axis=1)
        n_any = (~np.isnan(rt) | ~np.isnan(rg)).sum(axis=1)
        print("    steps compared per candidate: theta %d..%d, gamma %d..%d, either %d..%d" % (n_th.min(), n_th.max(), n_ga.min(), n_ga.max(),
                                                                                          n_any.min(), n_any.max()))
        assert n_any.min() >= 8, (tag, n_any)
        if dtype == "f64":
            assert n_th.min() >= 8 and n_ga.min() >= 8, (tag, n_th, n_ga)


# ---- cost terms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("which", ["w_theta", "w_gamma", "w_u"])
def test_one_cost_term_on_the_returned_trajectory(rv, orc, which, dtype):
    worst = 0.0
    for op in (0, 2, 4):
        row = rr.table()[op]
        kw = dict(ZERO_W)
        kw[which] = {"w_theta": 1.0, "w_gamma": 0.7, "w_u": 1e-6}[which]
        cfg = rv.MPCConfig(N=20, K=rr.K_TABLE, dtype=dtype, **kw)
        U, J, traj, _ = rollout(rv, cfg, rv.default_model(), row.state, row.U)
        ocfg = oracle_cfg(orc, cfg)
        for k in range(len(U)):
            want, bound = rr.cost_term_true(ocfg, which, U[k], traj[k], dtype)
            err = abs(float(rr.mpf(float(J[k])) - want))
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
    print("%s alone, %s: largest error / ((N + 3) eps J*) = %.3f" % (which, dtype, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_default_weight_cost_and_the_record(rv, orc, dtype):
    """J with the default weights on the returned nodes (tension and lowest point from cable_reference, with their bounds), and
    step()'s record against row arg-min J of rollout_costs, bit for bit."""
    worst = 0.0
    for op in (2, 4):
        row = rr.table()[op]
        cfg = rv.MPCConfig(N=20, K=8, dtype=dtype)
        U, J, traj, res = rollout(rv, cfg, rv.default_model(), row.state, row.U[:8], with_step=True)
        ocfg = oracle_cfg(orc, cfg)
        for k in range(len(U)):
            want, bound = rr.full_cost_true(ocfg, row.state, U[k], traj[k], dtype)
            worst = max(worst, abs(float(rr.mpf(float(J[k])) - want)) / bound)
        record_is_the_best_row(res, U, J, traj)
    print("default-weight J, %s: largest error / bound = %.3f" % (dtype, worst))
    assert worst <= 1.0
