"""The estimation kernels of csrc/util_kernels.h against the 50-digit references of tests/estimation_reference.py, through the
public entries: kabsch_velocity_transform, preprocess_signals, Engine.features_dd, compute_derivatives, extract_features_arrays,
rk4_integration and integrate_theta_gamma.

Every margin is the one test_estimation_reference_host.py fixes from the float64 oracle; none comes from a GPU run.  Each test
prints its largest ratio of error to bound (in units of the bound at m = 1) before it asserts.  Besides the bounds, every kernel
is run on a reordered or shortened input, and the rows that cannot see the change must keep their bits: a lane's result may not
depend on its place in the block or the grid."""
import functools

import numpy as np
import pytest
from mpmath import mp, mpf

import estimation_reference as er
import test_estimation_reference_host as host

pytestmark = pytest.mark.gpu

EPS = er.EPS


@pytest.fixture(scope="module")
def rv():
    import rovmpc
    return rovmpc


@pytest.fixture(scope="module")
def orc():
    from oracle import rovmpc_oracle
    return rovmpc_oracle


@pytest.fixture(scope="module")
def eng(rv):
    with rv.Engine(rv.MPCConfig(N=2, K=2)) as e:
        yield e


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- Kabsch ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kabsch_out(rv):
    """(v_out, R) of one call per M over the whole workspace, batch_gates off; made once."""
    cache = {}

    def get(M):
        if M not in cache:
            t = er.kabsch_table(M)
            cache[M] = rv.kabsch_velocity_transform(t.P, t.Q, t.v, batch_gates=False)
        return cache[M]
    return get


def _tags(t, family, *tags):
    return np.array([f.family == family and (not tags or f.tag in tags) for f in t.frames])


def _kabsch_ratios(t, R, v, idx=None):
    """(error / bound at m = 1) of R and of the R part of v_out, and the orthogonality defect, per frame."""
    eR, ev = er.kabsch_errors(t, R, v, idx)
    s = slice(None) if idx is None else idx
    kap = 1 + t.kappa[s]; v1 = np.abs(t.v[s]).sum(axis=1)
    return eR / (EPS * kap), (ev - 4 * EPS * v1) / (EPS * kap * v1), er.orthogonality_defect(R)


@pytest.mark.parametrize("M", er.MS)
def test_kabsch_whole_workspace(kabsch_out, rv, M):
    """Families (a)-(f) and (g) up to k = 100: R and v_out within the bounds, |R R^T - I| within the measured defect bound,
    det R > 0 on every decided frame; an undecided frame is all NaN or a matrix that meets the orthogonality check.  Then
    the same frames in reverse order: each frame keeps its bits, whatever its lane and block."""
    t = er.kabsch_table(M)
    v, R = kabsch_out(M)
    extreme = _tags(t, "g", "k=+400", "k=-400")                         # test_kabsch_extreme_scales
    dec = t.decided & ~extreme
    with np.errstate(all="ignore"):
        rR, rv_, defect = _kabsch_ratios(t, R, v)
        det = np.linalg.det(R)
    print("Kabsch M = %d: largest ratio R %.3f, v_out %.3f of m_R = %d; orthogonality defect %.3g of %.3g, over %d decided frames"
          % (M, rR[dec].max(), rv_[dec].max(), host.M_R, defect[dec].max(), host.DEFECT_BOUND, dec.sum()))
    bad = [(i, t.frames[i].family, t.frames[i].tag, rR[i], rv_[i], defect[i], det[i]) for i in np.nonzero(dec)[0]
           if not (rR[i] <= host.M_R and rv_[i] <= host.M_R and defect[i] <= host.DEFECT_BOUND and det[i] > 0)]
    assert not bad, bad[:10]
    und_nan = sum(bool(np.isnan(R[i]).all()) for i in np.nonzero(~t.decided)[0])
    print("Kabsch M = %d: %d undecided frames, %d of them NaN rows" % (M, (~t.decided).sum(), und_nan))
    for i in np.nonzero(~t.decided)[0]:
        all_nan = np.isnan(R[i]).all() and np.isnan(v[i]).all()
        assert all_nan or (defect[i] <= host.DEFECT_BOUND and det[i] > 0 and np.isfinite(v[i]).all()), (t.frames[i].tag, R[i], v[i])
    v2, R2 = rv.kabsch_velocity_transform(t.P[::-1], t.Q[::-1], t.v[::-1], batch_gates=False)
    assert _same(R2[::-1], R) and _same(v2[::-1], v)


@pytest.mark.parametrize("M", er.MS)
def test_kabsch_extreme_scales(kabsch_out, M):
    """Family (g).  Coordinates scaled by 2^(+-10) and 2^(+-100): R within the bound.  By 2^(+-400): every frame's output is
    within the bound or all NaN, never a finite matrix that fails the orthogonality check."""
    t = er.kabsch_table(M)
    v, R = kabsch_out(M)
    with np.errstate(all="ignore"):
        rR, rv_, defect = _kabsch_ratios(t, R, v)
        det = np.linalg.det(R)
    mid = _tags(t, "g", "k=+10", "k=-10", "k=+100", "k=-100")
    assert mid.sum() == 36 and (rR[mid] <= host.M_R).all() and (rv_[mid] <= host.M_R).all()
    bad, n_nan = [], 0
    for i in np.nonzero(_tags(t, "g", "k=+400", "k=-400"))[0]:
        if np.isnan(R[i]).all() and np.isnan(v[i]).all():
            n_nan += 1
        elif not (rR[i] <= host.M_R and rv_[i] <= host.M_R and defect[i] <= host.DEFECT_BOUND and det[i] > 0):
            bad.append((t.frames[i].tag, R[i].tolist(), defect[i]))
    print("Kabsch M = %d, coordinates scaled by 2^(+-400): %d of 18 frames NaN, %d finite and wrong" % (M, n_nan, len(bad)))
    assert not bad, bad[:4]


@pytest.mark.parametrize("T", [1, 128, 129, 48])
def test_kabsch_frame_does_not_depend_on_its_lane(rv, kabsch_out, T):
    t = er.kabsch_table(16)
    v0, R0 = kabsch_out(16)
    v, R = rv.kabsch_velocity_transform(t.P[:T], t.Q[:T], t.v[:T], batch_gates=False)
    v2, R2 = rv.kabsch_velocity_transform(t.P[:T][::-1], t.Q[:T][::-1], t.v[:T][::-1], batch_gates=False)
    assert _same(R2[::-1], R) and _same(v2[::-1], v)
    assert _same(R, R0[:T]) and _same(v, v0[:T])


def test_kabsch_motion_gate(rv):
    """batch_gates: |P - Q|_F just below 1e-6 is a NaN row, just above it a rotation within the bound."""
    rng = np.random.default_rng(99)
    for M in (4, 16):
        P = rng.normal(size=(6, M, 3)) * 0.5
        Q = np.empty_like(P)
        want = np.array([1 - 1e-6, 1 + 1e-6, 1 - 1e-9, 1 + 1e-9, 0.5, 2.0]) * 1e-6
        for i in range(6):
            d = rng.normal(size=(M, 3))
            Q[i] = P[i] + d * (want[i] / np.linalg.norm(d))
            norms = (np.linalg.norm(P[i] - Q[i]), float(np.sqrt(sum((x - y) ** 2 for x, y in zip(P[i].ravel(), Q[i].ravel())))))
            assert all((n < 1e-6) == (want[i] < 1e-6) and abs(n - 1e-6) > 1e-16 for n in norms), norms   # float64 norm on the intended side
        vv = rng.normal(size=(6, 3))
        v, R = rv.kabsch_velocity_transform(P, Q, vv, batch_gates=True)
        for i in range(6):
            if want[i] < 1e-6:
                assert np.isnan(R[i]).all() and np.isnan(v[i]).all(), i
                continue
            tr = er.kabsch_true(P[i], Q[i], vv[i])
            Rs = np.array(tr.R.tolist(), dtype=object); vs = np.array([tr.v[a] for a in range(3)], dtype=object)
            with mp.workdps(er.DPS):
                eR = max(float(abs(mpf(float(R[i, a, b])) - Rs[a, b])) for a in range(3) for b in range(3))
                ev = max(float(abs(mpf(float(v[i, a])) - vs[a])) for a in range(3))
            bR = host.M_R * EPS * (1 + tr.kappa)
            assert EPS * tr.kappa < er.UNDECIDED and eR <= bR and ev <= (bR + 4 * EPS) * np.abs(vv[i]).sum(), (M, i, eR / bR, tr.kappa)
        v2, R2 = rv.kabsch_velocity_transform(P, Q, vv, batch_gates=False)
        assert np.isfinite(R2).all() and _same(R2[want > 1e-6], R[want > 1e-6])


def test_kabsch_non_finite_marker_and_too_few_markers(rv, kabsch_out):
    """A NaN or Inf in any single coordinate of P or Q: that frame is a NaN row, and every other frame keeps the bits of a
    call without the poisoned frames.  M = 2: NaN rows (include/rovmpc.h: fewer than three markers)."""
    M = 4
    t = er.kabsch_table(M)
    P, Q, vv = t.P[:130].copy(), t.Q[:130].copy(), t.v[:130].copy()
    poisoned = []
    vals = (np.nan, np.inf, -np.inf)
    for n in range(2 * 3 * M):                                           # every coordinate of P, then of Q, in frames 3, 8, 13, ...
        i = 3 + 5 * n
        (P if n < 3 * M else Q)[i].reshape(-1)[n % (3 * M)] = vals[n % 3]
        poisoned.append(i)
    for i, arr in ((126, P), (127, Q), (128, P), (129, Q)):              # the block edge and the one-lane tail
        arr[i, 1, 2] = np.nan
        poisoned.append(i)
    keep = np.setdiff1d(np.arange(130), poisoned)
    for gates in (True, False):
        v, R = rv.kabsch_velocity_transform(P, Q, vv, batch_gates=gates)
        assert np.isnan(R[poisoned]).all() and np.isnan(v[poisoned]).all()
        vc, Rc = rv.kabsch_velocity_transform(P[keep], Q[keep], vv[keep], batch_gates=gates)
        assert _same(R[keep], Rc) and _same(v[keep], vc)
        if not gates:
            assert _same(Rc, kabsch_out(M)[1][keep])
    v, R = rv.kabsch_velocity_transform(t.P[:130, :2], t.Q[:130, :2], t.v[:130], batch_gates=False)
    assert R.shape == (130, 3, 3) and np.isnan(R).all() and np.isnan(v).all()


# ---- Gaussian filter --------------------------------------------------------------------------------------------------------

def _frame(t, theta, gamma):
    import pandas as pd
    return pd.DataFrame({"Time": t, "Theta": theta, "Gamma": gamma})


def _ratio(got, ref):
    e = er.err(got, ref.hi, ref.lo)
    with np.errstate(all="ignore"):
        r = np.where(ref.scale > 0, e / ref.scale, np.where(e == 0, 0.0, np.inf))
    return r


def test_gaussian_filter(rv):
    worst = 0.0
    for T, sigma in er.GAUSS_CASES:
        x, y = er.signal(T, 100 + T), er.signal(T, 150 + T)
        tt, th, ga = rv.preprocess_signals(_frame(er.times(T, "uniform", 0), x, y), sigma=sigma)
        for got, src in ((th, x), (ga, y)):
            r = _ratio(got, er.gaussian_reference(src, sigma))
            worst = max(worst, float(r.max()))
            assert (r <= host.M_GAUSS).all(), (T, sigma, float(r.max()), int(r.argmax()))
    print("Gaussian filter: largest ratio %.3f of m = %d" % (worst, host.M_GAUSS))


def test_gaussian_filter_prefixes(rv):
    """The first T' rows alone, T' around the 256-lane block edges: rows more than the radius (8) before the cut keep their bits."""
    T, radius = 513, 8
    x, y, t = er.signal(T, 100 + T), er.signal(T, 150 + T), er.times(T, "uniform", 0)
    _, th, ga = rv.preprocess_signals(_frame(t, x, y), sigma=2)
    for Tp in (255, 256, 257, 511, 512):
        _, th2, ga2 = rv.preprocess_signals(_frame(t[:Tp], x[:Tp], y[:Tp]), sigma=2)
        n = Tp - radius
        assert _same(th2[:n], th[:n]) and _same(ga2[:n], ga[:n]), Tp
        assert not _same(th2, th[:Tp])                                   # and the reflected end is indeed another sum


# ---- Savitzky-Golay and the chained gradients (features_dd, compute_derivatives) ----------------------------------------------

@functools.lru_cache(maxsize=None)
def _dd_case(T, kind, window, order):
    rng = np.random.default_rng(800 + T + window)
    t = er.times(T, kind, 300 + T)
    th, ga = er.signal(T, 600 + T), er.signal(T, 700 + T, 0.2)
    P0 = rng.normal(size=(T, 3)) * 300 + rng.uniform(-1e4, 1e4, size=3)
    P1 = P0 + rng.normal(size=(T, 3)) * 900
    V = rng.normal(size=(T, 3)) * 200
    return t, th, ga, P0, P1, V, er.derivative_chain(th, t, window, order), er.derivative_chain(ga, t, window, order)


def _check_chain(ch, smooth, d1, d2, label, worst):
    b = er.chain_bounds(ch, host.M_SAVGOL, host.M_GRAD)
    for k, (got, ref) in enumerate(((smooth, ch.smooth), (d1, ch.d1.ref), (d2, ch.d2.ref))):
        if got is None:
            continue
        e = er.err(got, ref.hi, ref.lo)
        # in units of the stage's own m = 1 bound (carried part included)
        unit = er.chain_bounds(ch, 1.0, 1.0)[k]
        worst[k] = max(worst[k], float((e / unit).max()))
        assert (e <= b[k]).all(), (label, k, float((e / b[k]).max()), int((e / b[k]).argmax()))


@pytest.mark.parametrize("T,window,order", er.SAVGOL_CASES)
def test_features_dd_smoothing_and_gradients(eng, T, window, order):
    """Columns 0, 1 (Savitzky-Golay) within m_savgol, columns 2, 3 and the targets within the bounds carried through one and
    two gradient passes; the gradient columns 6, 7, 11..13 against the 50-digit gradient of the kernel's own pass-1 columns
    4, 5, 8..10 (the values pass 2 reads); columns 4, 5 (v_sway, v_surge) against their own reference and columns 8..10 equal
    to V / 1000 bit for bit."""
    worst = [0.0, 0.0, 0.0]; worst_g = worst_s = 0.0
    for kind in ("uniform", "jitter"):
        t, th, ga, P0, P1, V, ch_th, ch_ga = _dd_case(T, kind, window, order)
        F, Y = eng.features_dd(P0, P1, V, t, th, ga, window, order)
        _check_chain(ch_th, F[:, 0], F[:, 2], Y[:, 0], (T, kind, "theta"), worst)
        _check_chain(ch_ga, F[:, 1], F[:, 3], Y[:, 1], (T, kind, "gamma"), worst)
        assert _same(F[:, 8:11], V / 1000)
        for col, ref in zip((4, 5), er.surge_sway_reference(P0, P1, V)):
            r = _ratio(F[:, col], ref)
            worst_s = max(worst_s, float(r.max()))
            assert (r <= host.M_SWAY).all(), (T, kind, col, float(r.max()), int(r.argmax()))
        for src, dst in ((4, 6), (5, 7), (8, 11), (9, 12), (10, 13)):
            r = _ratio(F[:, dst], er.gradient_reference(F[:, src], t).ref)
            worst_g = max(worst_g, float(r.max()))
            assert (r <= host.M_GRAD).all(), (T, kind, dst, float(r.max()), int(r.argmax()))
    print("features_dd T = %d window %d: largest ratio Savitzky-Golay %.3f (m = %d), first gradient %.3f, second gradient %.3f "
          "(of the carried bound at m = 1), single gradient pass %.3f (m = %d), v_sway / v_surge %.3f (m = %d)"
          % (T, window, worst[0], host.M_SAVGOL, worst[1], worst[2], worst_g, host.M_GRAD, worst_s, host.M_SWAY))


def test_savgol_hat_matrix_is_the_one_the_host_builds(eng):
    """A unit impulse at sample j returns column j of the hat matrix rows: the reference's restatement has the host's bits."""
    for window, order in ((11, 3), (21, 5)):
        W = er.savgol_hat(window, order)
        z = np.zeros((window, 3))
        got = np.empty((window, window))
        for j in range(window):
            F, _ = eng.features_dd(z, z + 1.0, z, np.arange(window) * 0.5, np.eye(window)[j], np.zeros(window), window, order)
            got[:, j] = F[:, 0]
        assert np.array_equal(got, W), float(np.abs(got - W).max())


@pytest.mark.parametrize("T", [11, 256, 257, 513])
def test_compute_derivatives(rv, T):
    """The third chained pass alone is returned here: within the bound carried from the smoothing through both gradients."""
    worst = [0.0, 0.0, 0.0]
    for kind in ("uniform", "jitter"):
        t, th, ga, _, _, _, ch_th, ch_ga = _dd_case(T, kind, 11, 3)
        ddt, ddg = rv.compute_derivatives(_frame(t, th, ga))
        _check_chain(ch_th, None, None, ddt, (T, kind, "theta"), worst)
        _check_chain(ch_ga, None, None, ddg, (T, kind, "gamma"), worst)
    print("compute_derivatives T = %d: largest ratio %.3f of the carried bound at m = 1" % (T, worst[2]))


def test_features_dd_prefixes(eng):
    """The first T' rows alone.  Pass-1 columns that read one row keep every row's bits; the smoothed columns those more than
    half a window before the cut; a single gradient pass those more than one row before it; the gradient of the smoothed
    columns and the targets one and two rows earlier than the smoothed columns."""
    T, window, half = 513, 11, 5
    t, th, ga, P0, P1, V, _, _ = _dd_case(T, "jitter", window, 3)
    F, Y = eng.features_dd(P0, P1, V, t, th, ga)
    for Tp in (255, 256, 257, 511, 512):
        F2, Y2 = eng.features_dd(P0[:Tp], P1[:Tp], V[:Tp], t[:Tp], th[:Tp], ga[:Tp])
        assert _same(F2[:, [4, 5, 8, 9, 10]], F[:Tp, [4, 5, 8, 9, 10]]), Tp
        n = Tp - half
        assert _same(F2[:n, :2], F[:n, :2]) and not _same(F2[:, :2], F[:Tp, :2]), Tp
        assert _same(F2[:Tp - 1, [6, 7, 11, 12, 13]], F[:Tp - 1, [6, 7, 11, 12, 13]]), Tp
        assert _same(F2[:n - 1, 2:4], F[:n - 1, 2:4]) and _same(Y2[:n - 2], Y[:n - 2]), Tp


# ---- the feature map ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", er.FEATURE_TS)
def test_extract_features(rv, T):
    P0, P1, V1, t, th, ga = er.feature_inputs(T)
    ref = er.features_reference(P0, P1, V1, t, th, ga)
    X = rv.extract_features_arrays(P0, P1, V1, t, th, ga)
    X16 = rv.extract_features_arrays(P0, P1, V1, t, th, ga, with_prev=False)
    assert X.shape == (T, 18) and X16.shape == (T, 16) and _same(X16, X[:, :16])
    assert _same(X[:, er.EXACT_COLS], ref.hi[:, er.EXACT_COLS])
    r = _ratio(X, ref)
    print("extract_features T = %d: largest ratio gradient columns %.3f of m = %d, unit vector / length / cosine %.3f of m = %d"
          % (T, r[:, 6:9].max(), host.M_GRAD, r[:, 9:14].max(), host.M_FEAT))
    assert (r[:, 6:9] <= host.M_GRAD).all(), np.argwhere(r[:, 6:9] > host.M_GRAD)[:5]
    assert (r[:, 9:14] <= host.M_FEAT).all(), np.argwhere(r[:, 9:14] > host.M_FEAT)[:5]
    assert (np.abs(X[:, 13]) <= 1).all() and (X[:, 12] >= 1e-5).all() and (X[:, 12] <= 10).all()      # the clips themselves


@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("kind", ["uniform", "jitter"])
def test_gradient_of_the_shortest_logs(rv, T, kind):
    """np.gradient with no interior row (T = 2) and with one (T = 3); features_dd needs a window of rows, the feature map does not."""
    P0, P1, V1, _, th, ga = er.feature_inputs(T, seed=4400 + T)
    t = er.times(T, kind, 300 + T)
    X = rv.extract_features_arrays(P0, P1, V1, t, th, ga)
    for a in range(3):
        r = _ratio(X[:, 6 + a], er.gradient_reference(V1[:, a], t).ref)
        assert (r <= host.M_GRAD).all(), (a, r)


def test_extract_features_prefixes(rv):
    T = 513
    P0, P1, V1, t, th, ga = er.feature_inputs(T)
    X = rv.extract_features_arrays(P0, P1, V1, t, th, ga)
    other = [c for c in range(18) if c not in (6, 7, 8)]
    for Tp in (255, 256, 257, 511, 512):
        X2 = rv.extract_features_arrays(P0[:Tp], P1[:Tp], V1[:Tp], t[:Tp], th[:Tp], ga[:Tp])
        assert _same(X2[:, other], X[:Tp, other]) and _same(X2[:Tp - 1, 6:9], X[:Tp - 1, 6:9]), Tp


# ---- replay increments --------------------------------------------------------------------------------------------------------

def test_replay_increments_across_block_edges(rv, orc, golden_dir, equations):
    """rk4_integration and integrate_theta_gamma at T around the 128-lane blocks of replay_increments_kernel, against the
    oracle's float64 replay at test_replay_integrators' tolerance; a shorter log keeps the bits of the longer one's start."""
    import os
    from conftest import chosen_row
    g = np.load(os.path.join(golden_dir, "kat_replay.npz"))
    th0, ga0 = float(g["theta0"]), float(g["gamma0"])
    et, eg = chosen_row(equations, "dtheta_dt")["sympy_format"], chosen_row(equations, "dgamma_dt")["sympy_format"]
    mt, mg = rv.SymbolicRegressor(et), rv.SymbolicRegressor(eg)
    ot, og = orc.SymbolicModel(et), orc.SymbolicModel(eg)
    out = {}
    for T in er.REPLAY_TS:
        X, t = er.replay_rows(g["Xs"], g["time"], T)
        rk_t, rk_g = rv.rk4_integration(mt, X, t, th0), rv.rk4_integration(mg, X, t, ga0)
        eu_t, eu_g = rv.integrate_theta_gamma(mt, mg, X, t, th0, ga0)
        np.testing.assert_allclose(rk_t, orc.rk4_replay(ot.predict, X, t, th0), rtol=er.REPLAY_RTOL)
        np.testing.assert_allclose(rk_g, orc.rk4_replay(og.predict, X, t, ga0), rtol=er.REPLAY_RTOL)
        w_t, w_g = orc.euler_replay(ot.predict, og.predict, X, t, th0, ga0)
        np.testing.assert_allclose(eu_t, w_t, rtol=er.REPLAY_RTOL); np.testing.assert_allclose(eu_g, w_g, rtol=er.REPLAY_RTOL)
        out[T] = (rk_t, rk_g, eu_t, eu_g)
    for T in er.REPLAY_TS[:-1]:
        for a, b in zip(out[T], out[257]):
            assert _same(a, b[:T]), T
