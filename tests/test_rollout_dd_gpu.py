"""The second-order (generation-3) rollouts -- integrate_dd, integrate_dd_jit and the features_dd rows of phase 2 -- against
the 50-digit global reference of tests/rollout_dd_reference.py: every decided node of every candidate within M_DD x the bound
propagated to it, in fp64 and fp32, on the interpreter and hiprtc paths, in every velocity transform and both integrators,
from N = 1 and K = 1 to ragged workgroups; bit-identity across candidates_per_block and duplicates, the NaN candidate, step()'s
record, the cost read off the returned nodes.  Every case is one rollout_costs(state, U, return_traj=True) call (and a step()
where the record is checked); each test prints its largest ratio before it asserts."""
import functools

import numpy as np
import pytest

import rollout_dd_reference as rd
import rollout_reference as rr
from rollout_gpu_helpers import oracle_cfg, oracle_model_named, rand_rtab, record_is_the_best_row, rollout

pytestmark = pytest.mark.gpu

ZERO_W = dict(w_theta=0.0, w_gamma=0.0, w_u=0.0, w_T=0.0, w_taut=0.0, w_floor=0.0)
OTHER_ROWS = [(9, 8), (14, 9), (22, 18), (4, 16)]
DIVIDES_BY_VX = [(9, 8), (14, 9), (22, 18)]
ORDINARY_ROW = 0
N_TABLE = 8


@pytest.fixture(scope="module")
def rv():
    import rovmpc
    return rovmpc


@pytest.fixture(scope="module")
def orc():
    from oracle import rovmpc_oracle
    return rovmpc_oracle


def config(rv, N, K, dtype, jit=True, **kw):
    return rv.MPCConfig(N=N, K=K, dtype=dtype, jit=jit, feature_map=rv.FEATURES_GEN3, **kw)


def path_of(jit):
    return "jit" if jit else "interpreter"


def oracle_nodes(rv, orc, cfg, model, state, U, Rtab=None):
    """The oracle's J and trajectory on the inputs as the kernel reads them (state and controls rounded to the type)."""
    st = np.asarray(state, dtype=np.float64).astype(cfg.np_dtype).astype(np.float64)
    J, traj, _ = orc.rollout_vec_dd(oracle_cfg(orc, cfg), oracle_model_named(orc, model), orc.MPCState.from_array(st),
                                    np.asarray(U, dtype=np.float64), Rtab)
    return J, traj


def check_nodes(rv, orc, cfg, model, state, U, Rtab=None, what="", path=None, skip=(), with_step=False, need_decided=True):
    """One rollout_costs call, every decided node of every candidate (but those in `skip`) against the reference; with_step:
    step()'s record is row arg-min J of that call, bit for bit."""
    U, J, traj, res = rollout(rv, cfg, model, state, U, Rtab, with_step=with_step, path=path)
    rt, rg = rd.ratios(oracle_cfg(orc, cfg), model, state, U, traj, cfg.dtype, Rtab)
    keep = np.array([k not in skip for k in range(len(U))])
    w = rd.worst(rt[keep], rg[keep])
    print("%s %s: largest ratio %.3f of M_DD %.2f (theta %.3f, gamma %.3f; decided %d + %d of %d nodes)"
          % (what, cfg.dtype, w, rd.M_DD, rd.worst(rt[keep], rt[keep]), rd.worst(rg[keep], rg[keep]), (~np.isnan(rt[keep])).sum(),
             (~np.isnan(rg[keep])).sum(), rt[keep].size))
    if need_decided:
        assert (~np.isnan(rt[keep])).any() and (~np.isnan(rg[keep])).any(), what
    assert w <= rd.M_DD, (what, w)
    if with_step:
        record_is_the_best_row(res, U, J, traj)
    return U, J, traj, rt, rg


# ---- sweep -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sweep_row(i, dtype, jit):
    import rovmpc as rv
    from oracle import rovmpc_oracle as orc
    row = rd.table_dd(N_TABLE, dtype)[i]
    return check_nodes(rv, orc, config(rv, N_TABLE, rd.K_TABLE, dtype, jit), rv.generation3_model(), row.state, row.U,
                       what="sweep %s %s" % (path_of(jit), row.tag), path=path_of(jit), skip=(rd.NAN_CANDIDATE,) if i == rd.NAN_ROW else ())


@pytest.mark.parametrize("jit", [True, False])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("i", range(len(rd.table_dd(N_TABLE))))
def test_sweep_of_the_workspace(i, dtype, jit):
    """The whole table on the chosen rows (complexity 6 / 5): composed velocity transform, RK4, N = 8, K = 19, dt = 1/60."""
    _sweep_row(i, dtype, jit)


@pytest.mark.parametrize("jit", [True, False])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_specials_of_the_sweep(rv, orc, dtype, jit):
    """The NaN candidate has the oracle's NaN nodes and J = +inf while the rest of its workgroup stays within bound; duplicate
    candidates return the same bits."""
    U, J, traj, rt, rg = _sweep_row(rd.NAN_ROW, dtype, jit)
    c = rd.NAN_CANDIDATE
    assert np.isnan(traj[c, 1:]).all() and np.isposinf(J[c])
    row = rd.table_dd(N_TABLE, dtype)[rd.NAN_ROW]
    _, trajo = oracle_nodes(rv, orc, config(rv, N_TABLE, rd.K_TABLE, dtype, jit), rv.generation3_model(), row.state, U)
    assert np.array_equal(np.isnan(traj), np.isnan(trajo))
    others = [k for k in range(16) if k != c]
    assert np.isfinite(J[others]).all() and np.isfinite(traj[others]).all()
    assert not np.isnan(rt[others]).all() and not np.isnan(rg[others]).all() and rd.worst(rt[others], rg[others]) <= rd.M_DD
    for i in range(len(rd.table_dd(N_TABLE, dtype))):
        U, J, traj, _, _ = _sweep_row(i, dtype, jit)
        assert np.array_equal(U[0], U[-1])
        assert J[0] == J[-1] and np.array_equal(traj[0], traj[-1]), rd.table_dd(N_TABLE, dtype)[i].tag


@pytest.mark.parametrize("jit", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_candidates_per_block_does_not_change_the_bits(rv, orc, dtype, jit):
    """One candidate per workgroup against 16.  On the interpreter both run the library's one build of the kernel: the same J
    and trajectory bits.  On the hiprtc path they are two modules (16 per workgroup is built with that and N as literals),
    and FMA contraction is chosen per build (the numerical liberties): bits are no law across them
    -- measured in fp32, J differs in the last place for 3 of 19 candidates, 58.51644 against 58.516468 --, so there each
    build is held to the bound on its own."""
    row = rd.table_dd(N_TABLE, dtype)[rd.BIG_ROW]
    out = [rollout(rv, config(rv, N_TABLE, rd.K_TABLE, dtype, jit, candidates_per_block=ck), rv.generation3_model(), row.state, row.U,
                   path=path_of(jit)) for ck in (1, 16)]
    if not jit:
        assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    for ck in ((1, 16) if jit else (1,)):
        check_nodes(rv, orc, config(rv, N_TABLE, rd.K_TABLE, dtype, jit, candidates_per_block=ck), rv.generation3_model(), row.state, row.U,
                    what="%d per workgroup, %s, %s" % (ck, path_of(jit), row.tag), path=path_of(jit))


# ---- modes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jit", [True, False])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("vt_mode", [0, 1, 2])
@pytest.mark.parametrize("i", [0, rd.BIG_ROW])
def test_modes(rv, orc, i, vt_mode, integrator, dtype, jit):
    """A small-rate row and the (-2.0, 1.5) one in every velocity transform, RK4 and the double Euler, N = 12."""
    row = rd.table_dd(12, dtype)[i]
    check_nodes(rv, orc, config(rv, 12, 8, dtype, jit, vt_mode=vt_mode, integrator=integrator), rv.generation3_model(), row.state, row.U[:8],
                rand_rtab(12) if vt_mode == 2 else None, what="modes vt=%d integ=%d %s %s" % (vt_mode, integrator, path_of(jit), row.tag),
                path=path_of(jit))


# ---- other rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("i", [rd.VX0_ROW, ORDINARY_ROW])
@pytest.mark.parametrize("ct,cg", OTHER_ROWS)
def test_other_rows(rv, orc, ct, cg, i, dtype):
    """Division by V_x, nested sines, the 'gama' variable.  The oracle's NaN / inf pattern is the kernel's; on the ordinary row
    at least half of the candidates are decided.  On the V_x = 0 row the rows that divide by V_x are counted apart: an exact
    zero divisor in fp64 (every node NaN on both sides), a divisor within its uncertainty of zero in fp32 (nothing decided)."""
    row = rd.table_dd(N_TABLE, dtype)[i]
    model = rv.generation3_model(ct, cg)
    cfg = config(rv, N_TABLE, rd.K_TABLE, dtype)
    apart = i == rd.VX0_ROW and (ct, cg) in DIVIDES_BY_VX
    U, J, traj, rt, rg = check_nodes(rv, orc, cfg, model, row.state, row.U, what="rows (%d, %d) %s" % (ct, cg, row.tag), path="jit",
                                     need_decided=not apart)
    Jo, trajo = oracle_nodes(rv, orc, cfg, model, row.state, U)
    assert np.array_equal(np.isnan(traj), np.isnan(trajo)) and np.array_equal(np.isinf(traj), np.isinf(trajo))
    assert np.array_equal(np.isposinf(J), np.isposinf(Jo))
    if apart and dtype == "f64":
        assert np.isnan(traj[:, 1:, 0]).all()
    if i == ORDINARY_ROW:
        decided = (~np.isnan(rt)).any(axis=1) & (~np.isnan(rg)).any(axis=1)
        assert decided.sum() * 2 >= len(U), decided


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,dtype,dt", [(N, K, dtype, 1 / 60) for N, K in rd.SHAPES for dtype in ("f64", "f32")] + [(40, 3, "f64", 1 / 240)])
def test_shapes(rv, orc, N, K, dtype, dt):
    """A single candidate and step (the purely local check, the edge rule of node 0 alone); a ragged workgroup; odd sizes over
    several workgroups; the longest horizon of the list at the data rate of 240 Hz.  step()'s record is the checked call's best
    row, bit for bit."""
    state, U = rd.shape_case(N, K, dtype)
    _, _, _, rt, rg = check_nodes(rv, orc, config(rv, N, K, dtype, dt=dt), rv.generation3_model(), state, U,
                                  what="shape N=%d K=%d" % (N, K), path="jit", with_step=True)
    if N == 1:
        assert not np.isnan(rt).any() and not np.isnan(rg).any()            # the single step is decided for every candidate


# ---- dt = 0.05 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("vt_mode", [0, 1])
@pytest.mark.parametrize("ct,cg", [(None, None), (9, 8)])
def test_dt_of_survey_and_verdict(rv, orc, ct, cg, vt_mode, dtype):
    """dt = 0.05 s, N = 8 (beyond it the propagated bound grows by 1e3 and more): the chosen rows and a pair that divides by V_x."""
    row = rd.table_dd(N_TABLE, dtype)[rd.BIG_ROW]
    check_nodes(rv, orc, config(rv, N_TABLE, 8, dtype, dt=0.05, vt_mode=vt_mode), rv.generation3_model(ct, cg), row.state, row.U[:8],
                what="dt=0.05 vt=%d rows (%s, %s) %s" % (vt_mode, ct, cg, row.tag), path="jit")


# ---- cost terms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("which", ["w_theta", "w_gamma", "w_u"])
def test_one_cost_term_on_the_returned_trajectory(rv, orc, which, dtype):
    worst = 0.0
    for i in (0, rd.BIG_ROW):
        row = rd.table_dd(N_TABLE, dtype)[i]
        kw = dict(ZERO_W)
        kw[which] = {"w_theta": 1.0, "w_gamma": 0.7, "w_u": 1e-6}[which]
        cfg = config(rv, N_TABLE, 8, dtype, **kw)
        U, J, traj, _ = rollout(rv, cfg, rv.generation3_model(), row.state, row.U[:8])
        ocfg = oracle_cfg(orc, cfg)
        for k in range(len(U)):
            want, bound = rr.cost_term_true(ocfg, which, U[k], traj[k], dtype)
            err = abs(float(rr.mpf(float(J[k])) - want))
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
    print("%s alone, %s: largest error / ((N + 3) eps J*) = %.3f" % (which, dtype, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_default_weight_cost_and_the_record(rv, orc, dtype):
    """J with the default weights on the returned nodes (the cost law is the first-order rollout's: tension and lowest point
    from cable_reference, with their bounds), and step()'s record against row arg-min J of rollout_costs, bit for bit."""
    worst = 0.0
    for i in (0, rd.BIG_ROW):
        row = rd.table_dd(N_TABLE, dtype)[i]
        cfg = config(rv, N_TABLE, 8, dtype)
        U, J, traj, res = rollout(rv, cfg, rv.generation3_model(), row.state, row.U[:8], with_step=True)
        ocfg = oracle_cfg(orc, cfg)
        for k in range(len(U)):
            want, bound = rr.full_cost_true(ocfg, row.state, U[k], traj[k], dtype)
            worst = max(worst, abs(float(rr.mpf(float(J[k])) - want)) / bound)
        record_is_the_best_row(res, U, J, traj)
    print("default-weight J, %s: largest error / bound = %.3f" % (dtype, worst))
    assert worst <= 1.0
