"""The one-step reference of the rollout (tests/rollout_reference.py) checked on the CPU: the margin M_STEP measured on the
float64 oracle, the reference against the scalar oracle, how much of the workspace is decided, which mechanisms of the
theta chain the workspace reaches, and that the bound rejects NumPy restatements of the step that break the law in one place."""
import numpy as np
import pytest

import rollout_reference as rr
from oracle import rovmpc_oracle as orc


@pytest.fixture(scope="module")
def model(oracle_model):
    return oracle_model


@pytest.fixture(scope="module")
def oracle_sweep(model):
    """Per table row: the oracle's trajectory and its one-step ratios against step_true on its own nodes."""
    cfg = orc.MPCConfig(N=20)
    out = []
    for row in rr.table():
        _, traj, _ = orc.rollout_vec(cfg, model, orc.MPCState.from_array(row.state), row.U)
        out.append((row, traj) + rr.step_ratios(cfg, model, row.state, row.U, traj))
    return out


def test_margin_is_measured_on_the_oracle(oracle_sweep):
    wt = max(float(np.nanmax(rt)) for _, _, rt, _, _ in oracle_sweep)
    wg = max(float(np.nanmax(rg)) for _, _, _, rg, _ in oracle_sweep)
    print("largest one-step ratio of the float64 oracle: theta %.3f gamma %.3f, M_STEP %.2f" % (wt, wg, rr.M_STEP))
    assert rr.M_STEP >= 4.0
    assert max(wt, wg) <= rr.M_STEP / 2
    assert max(wt, wg) > 0.02                                   # the scale is not orders of magnitude above a plain float64 run


def test_step_true_equals_the_scalar_oracle(model):
    for i, (vt, prev, integ) in ((2, (1, 0, 0)), (4, (1, 1, 0)), (10, (0, 0, 1)), (12, (2, 0, 0))):
        row = rr.table()[i]
        cfg = orc.MPCConfig(N=5, vt_mode=vt, prev_mode=prev, integrator=integ)
        U = row.U[:3, :5]
        Rtab = np.stack([np.linalg.qr(np.random.default_rng(5 + n).standard_normal((3, 3)))[0] for n in range(5)]) if vt == 2 else None
        _, traj, _ = orc.rollout_scalar(cfg, model, orc.MPCState.from_array(row.state), U, Rtab)
        for k in range(3):
            for n in range(5):
                th, ga = rr.step_true(cfg, model, row.state, U[k], traj[k], n, Rtab)
                assert float(th) == pytest.approx(traj[k, n + 1, 0], rel=1e-12, abs=1e-15)
                assert float(ga) == pytest.approx(traj[k, n + 1, 1], rel=1e-12, abs=1e-15)


def test_most_of_the_workspace_is_decided(oracle_sweep):
    """At most 5 % of a row's steps are undecided and no row is undecided in full (the NaN candidate is a special of the GPU
    tests, not a step: it is left out of the count)."""
    for i, (row, traj, rt, rg, _) in enumerate(oracle_sweep):
        keep = np.ones(len(rt), bool)
        if i == rr.NAN_ROW:
            keep[rr.NAN_CANDIDATE] = False
            assert np.isnan(rt[rr.NAN_CANDIDATE]).all()
        for r in (rt[keep], rg[keep]):
            assert np.isnan(r).mean() <= 0.05, row.tag
            assert not np.isnan(r).all(), row.tag


def test_the_workspace_reaches_the_mechanisms_of_the_theta_chain(oracle_sweep, model):
    d = np.concatenate([dth[np.isfinite(dth)] for _, _, _, _, dth in oracle_sweep])
    assert (d >= 2.0 ** -6).mean() >= 0.10 and (d < 2.0 ** -6).mean() >= 0.10
    assert all(row.U.shape[1] >= 17 for row, *_ in oracle_sweep)            # step 16 re-anchors the angle addition
    mean, scale = model.mean, model.scale
    huge = rr.table()[rr.HUGE_ROW]
    assert np.max(np.abs((huge.U[..., 0] - mean[3]) / scale[3])) > rr.TRIG_FAST_LIMIT
    assert all(len(row.U) == rr.K_TABLE for row, *_ in oracle_sweep)
    ops = {tuple(row.state[12:14]) for row, *_ in oracle_sweep}
    assert ops == set(rr.OPERATING)


# ---- mutants ---------------------------------------------------------------------------------------------------------------

def _rod(v, axis, s, c):
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    return v * c[:, None] + np.cross(axis, v) * s[:, None] + axis * np.sum(axis * v, axis=-1, keepdims=True) * (1 - c[:, None])


def numpy_rollout(cfg, model, state, U, mutant=None):
    """oracle.rollout_vec's (theta, gamma) trajectory restated (generation-1 map, composed velocity transform), with one
    deliberate deviation from the law."""
    K, N, _ = U.shape
    mean, scale, h = model.mean, model.scale, cfg.dt
    st = orc.MPCState.from_array(state)
    P0 = st.P0
    P, V, A = (np.tile(x, (K, 1)) for x in (st.P1, st.V1, st.A1))
    th, ga = np.full(K, st.theta), np.full(K, st.gamma)
    thm, gam = np.full(K, st.theta_prev), np.full(K, st.gamma_prev)
    thmm, gamm = thm.copy(), gam.copy()
    traj = np.zeros((K, N + 1, 2)); traj[:, 0, 0] = th; traj[:, 0, 1] = ga
    xs_n = orc._exo_features_vec(P0, P, V, A, mean, scale)
    h6 = float(np.float32(h / 6)) if mutant == "h6_f32" else h / 6
    hold = cfg.prev_mode == 1 or mutant == "hold"

    def f(cols):
        return (np.broadcast_to(np.asarray(model.f_theta(cols), float), (K,)), np.broadcast_to(np.asarray(model.f_gamma(cols), float), (K,)))

    def integrate(Vn, xs_n, a16, b16, a17, b17):
        An = (Vn - V) / h
        xs_n1 = orc._exo_features_vec(P0, P + (cfg.v_scale * h) * Uw, Vn, An, mean, scale)
        s16a, s16b = (a16 - mean[16]) / scale[16], (b16 - mean[16]) / scale[16]
        s17a, s17b = (a17 - mean[17]) / scale[17], (b17 - mean[17]) / scale[17]

        def stage(yth, yga, c):
            exo = xs_n if c == 0.0 else xs_n1 if c == 1.0 else (xs_n if mutant == "noavg" else (xs_n + xs_n1) / 2)
            if hold or c == 0.0:
                p16, p17 = s16a, s17a
            elif c == 1.0:
                p16, p17 = s16b, s17b
            else:
                p16, p17 = (s16a + s16b) / 2, (s17a + s17b) / 2
            return f([exo[:, i] for i in range(14)] + [(yth - mean[14]) / scale[14], (yga - mean[15]) / scale[15], p16, p17])

        k1 = stage(th, ga, 0.0)
        k2 = stage(th + 0.5 * h * k1[0], ga + 0.5 * h * k1[1], 0.5)
        k3 = k2 if mutant == "k3_is_k2" else stage(th + 0.5 * h * k2[0], ga + 0.5 * h * k2[1], 0.5)
        k4 = stage(th + h * k3[0], ga + h * k3[1], 1.0)
        return (th + h6 * (k1[0] + 2 * k2[0] + 2 * k3[0] + k4[0]), ga + h6 * (k1[1] + 2 * k2[1] + 2 * k3[1] + k4[1]), An, xs_n1)

    with np.errstate(all="ignore"):
        for n in range(N):
            Uw = U[:, n, :]
            tha, gaa = orc._axes_vec(P - P0)

            def vt(t, g):
                s, c = np.sin(t), np.cos(t)
                if mutant == "sincos_1e-12":
                    s, c = s * (1 + 1e-12), c * (1 - 1e-12)
                return _rod(_rod(Uw, gaa, np.sin(-g), np.cos(-g)), tha, s, c)

            d = (thmm, thm, gamm, gam) if mutant == "delay_late" else (thm, th, gam, ga)
            Vn = vt(th, ga)
            th_n, ga_n, An, xs_n1 = integrate(Vn, xs_n, d[0], d[1], d[2], d[3])
            if mutant == "vt_theta_next":
                Vn = vt(th_n, ga)
                th_n, ga_n, An, xs_n1 = integrate(Vn, xs_n, d[0], d[1], d[2], d[3])
            thmm, gamm = thm, gam
            thm, gam, th, ga = th, ga, th_n, ga_n
            P, V, A, xs_n = P + (cfg.v_scale * h) * Uw, Vn, An, xs_n1
            traj[:, n + 1, 0] = th; traj[:, n + 1, 1] = ga
    return traj


MUTANTS = ("hold", "noavg", "k3_is_k2", "vt_theta_next", "sincos_1e-12", "delay_late", "h6_f32")


@pytest.fixture(scope="module")
def mutant_rows():
    t = rr.table(8)
    return [rr.Row(t[i].tag, t[i].state, t[i].U[:6]) for i in (2, 4)]          # the operating points (0.6, -0.6) and (1.5, 0.3)


def test_the_restatement_itself_is_within_the_bound(model, mutant_rows):
    cfg = orc.MPCConfig(N=8)
    for row in mutant_rows:
        traj = numpy_rollout(cfg, model, row.state, row.U)
        _, want, _ = orc.rollout_vec(cfg, model, orc.MPCState.from_array(row.state), row.U)
        np.testing.assert_allclose(traj, want, rtol=1e-12, atol=1e-15)
        rt, rg, _ = rr.step_ratios(cfg, model, row.state, row.U, traj)
        assert rr.worst(rt, rg) <= rr.M_STEP / 2


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_bound_rejects_a_step_that_breaks_the_law(model, mutant_rows, mutant):
    cfg = orc.MPCConfig(N=8)
    for row in mutant_rows:
        traj = numpy_rollout(cfg, model, row.state, row.U, mutant)
        rt, rg, _ = rr.step_ratios(cfg, model, row.state, row.U, traj)
        w = rr.worst(rt, rg)
        print("%s on %s: largest ratio %.3g" % (mutant, row.tag, w))
        assert w > rr.M_STEP, (mutant, row.tag, w)
