"""The global reference of the second-order rollout (tests/rollout_dd_reference.py) checked on the CPU: the reference against
both flavours of the oracle, the margin M_DD measured on the float64 oracle, how much of the workspace is decided in fp64 and
fp32, the Jacobian of the step map against a direct difference of two trajectories, and that the bound rejects restatements of
the law that are wrong in one place."""
import functools

import mpmath as mp
import numpy as np
import pytest

import rollout_dd_reference as rd
from oracle import rovmpc_oracle as orc

N_TABLE = 8


def cfg_of(N, **kw):
    return orc.MPCConfig(N=N, feature_map=2, **kw)


def floats(ref):
    return np.array([[float(t), float(g)] for t, g in zip(ref.th, ref.ga)])


@functools.lru_cache(maxsize=None)
def sweep(fmt):
    """Per table row: the references of the default set-up (rows 6 / 5, composed transform, RK4, dt = 1/60)."""
    cfg, model = cfg_of(N_TABLE), rd.oracle_model_dd()
    return [rd.trajectory_true(cfg, model, row.state, row.U, fmt) for row in rd.table_dd(N_TABLE, fmt)]


@functools.lru_cache(maxsize=None)
def oracle_ratios():
    cfg, model = cfg_of(N_TABLE), rd.oracle_model_dd()
    sweep("f64")
    out = []
    for row in rd.table_dd(N_TABLE):
        _, traj, _ = orc.rollout_vec_dd(cfg, model, orc.MPCState.from_array(row.state), row.U)
        out.append(rd.ratios(cfg, model, row.state, row.U, traj))
    return out


def test_reference_equals_both_oracles_in_float64():
    model, N = rd.oracle_model_dd(), 5
    Rtab = np.stack([np.linalg.qr(np.random.default_rng(5 + n).standard_normal((3, 3)))[0] for n in range(N)])
    for i, vt, integ in ((0, 1, 0), (3, 1, 1), (2, 0, 0), (8, 0, 1), (4, 2, 0), (6, 1, 0)):
        row = rd.table_dd(N)[i]
        cfg, U = cfg_of(N, vt_mode=vt, integrator=integ), row.U[:3]
        st = orc.MPCState.from_array(row.state)
        _, vec, _ = orc.rollout_vec_dd(cfg, model, st, U, Rtab if vt == 2 else None)
        sca = orc.rollout_scalar_dd(cfg, model, st, U, Rtab if vt == 2 else None)
        for k in range(3):
            ref = floats(rd.RolloutDD(cfg, model, row.state, U[k], "f64", Rtab if vt == 2 else None).trajectory(bound=False))
            np.testing.assert_allclose(ref, vec[k], rtol=1e-11, atol=1e-14, err_msg=row.tag)
            np.testing.assert_allclose(ref, sca[k], rtol=1e-11, atol=1e-14, err_msg=row.tag)


def test_margin_is_measured_on_the_oracle():
    wt = max(rd.worst(rt, rt) for rt, _ in oracle_ratios())
    wg = max(rd.worst(rg, rg) for _, rg in oracle_ratios())
    print("largest ratio of the float64 oracle to the propagated bound: theta %.3f gamma %.3f, M_DD %.2f" % (wt, wg, rd.M_DD))
    assert rd.M_DD >= 4.0
    assert max(wt, wg) <= rd.M_DD / 2
    assert max(wt, wg) > 0.02                                   # the bound is not orders of magnitude above a plain float64 run


@pytest.mark.parametrize("fmt,cap", [("f64", 0.90), ("f32", 0.50)])
def test_most_of_the_workspace_is_decided(fmt, cap):
    """Per table row the decided share of the (candidate, node) pairs, theta and gamma each; the NaN candidate is counted apart
    (nothing of it is decided)."""
    for i, (row, refs) in enumerate(zip(rd.table_dd(N_TABLE, fmt), sweep(fmt))):
        keep = [k for k in range(len(refs)) if not (i == rd.NAN_ROW and k == rd.NAN_CANDIDATE)]
        sh_t = np.mean([(~refs[k].und_th[1:]).mean() for k in keep])
        sh_g = np.mean([(~refs[k].und_ga[1:]).mean() for k in keep])
        print("%s %s: decided theta %.3f gamma %.3f" % (fmt, row.tag, sh_t, sh_g))
        assert sh_t >= cap and sh_g >= cap, (fmt, row.tag, sh_t, sh_g)
        if i == rd.NAN_ROW:
            nan = refs[rd.NAN_CANDIDATE]
            assert nan.und_th[1:].all() and nan.und_ga[1:].all()


@pytest.mark.parametrize("fmt", ["f64", "f32"])
def test_single_step_cases_are_decided_in_full(fmt):
    """N = 1: the purely local check, on the inputs of the shape tests (no axis branch is near its threshold there)."""
    for N, K in rd.SHAPES:
        if N == 1:
            state, U = rd.shape_case(N, K, fmt)
            refs = rd.trajectory_true(cfg_of(1), rd.oracle_model_dd(), state, U.astype(rd.er.FMT[fmt].np), fmt)
            assert all(not r.und_th[1] and not r.und_ga[1] for r in refs), (N, K)


def test_jacobian_equals_a_difference_of_two_trajectories():
    """One entry of z_n moved by 1e-9 of itself: the step's difference over the shift is that column of |Phi_n|; and a shifted
    start stays, over the horizon, within the product of the |Phi_n| (first order, entries in absolute value)."""
    model, N = rd.oracle_model_dd(), 4
    for i, vt in ((0, 1), (3, 0)):
        row = rd.table_dd(N)[i]
        ro = rd.RolloutDD(cfg_of(N, vt_mode=vt), model, row.state, row.U[0])
        ro.trajectory()
        with mp.workdps(rd.DPS + 10):
            z = ro.zs[1]
            Phi = ro.jacobian(1, z)
            base = ro.step(1, z)[0]
            for j in range(len(z)):
                d = abs(z[j]) * mp.mpf(10) ** -9 if z[j] != 0 else mp.mpf(10) ** -9
                zz = list(z); zz[j] = z[j] + d
                got = [float(abs(a - b) / d) for a, b in zip(ro.step(1, zz)[0], base)]
                np.testing.assert_allclose(got, Phi[:, j], rtol=1e-6, atol=1e-30)
            shift = np.array([1e-9 if j < 4 else 0.0 for j in range(len(z))])
            zz = [a + mp.mpf(s) for a, s in zip(ro.zs[0], shift)]
            bound = shift.copy()
            for n in range(N):
                bound = ro.jacobian(n, ro.zs[n]) @ bound
                zz = ro.step(n, zz)[0]
            diff = np.array([float(abs(a - b)) for a, b in zip(zz, ro.zs[N])])
            assert np.all(diff <= bound * (1 + 1e-6)) and np.all(diff[:4] >= 1e-3 * bound[:4]), (row.tag, diff, bound)


@pytest.mark.parametrize("mutate", ["weights", "midpoint", "edge"])
def test_a_law_broken_in_one_place_leaves_the_bound(mutate):
    """RK4 weights (1, 2 + 1e-7, 2, 1), the level the 1e-8 comparison with the float64 oracle lets pass; the midpoint stages on
    the row of node n; the edge rule of node 0 on nodes 0 and 2."""
    model, N, worst = rd.oracle_model_dd(), N_TABLE, []
    for i in (0, 3):
        row = rd.table_dd(N)[i]
        cfg, U = cfg_of(N, vt_mode=0), row.U[:4]
        traj = np.stack([floats(rd.RolloutDD(cfg, model, row.state, u).trajectory(mutate=mutate, bound=False)) for u in U])
        rt, rg = rd.ratios(cfg, model, row.state, U, traj)
        worst.append(rd.worst(rt, rg))
        print("%s, %s: largest ratio %.3g (M_DD %.2f)" % (mutate, row.tag, worst[-1], rd.M_DD))
    assert min(worst) > 100 * rd.M_DD
